/*
 * ssad.h -- C ABI of libssad_hip.so, the MI355X (gfx950) kernels behind the
 * self-supervised anomaly-detection hot path.
 *
 * The reference (gabry1998/Self-Supervised-Anomaly-Detection) is pure Python and has no
 * FFI of its own: its numerics are PyTorch / torchvision / scikit-learn calls.  Each entry
 * point below replaces one such call site (cited as path:line relative to the reference
 * root).  Conventions:
 *   - plain pointers + sizes, no torch types; every pointer is a DEVICE pointer unless
 *     the name ends in _host;
 *   - the caller owns every buffer (inputs, outputs, workspaces);
 *   - `stream` is a hipStream_t passed as void*; launches are asynchronous on it and the
 *     library never synchronises;
 *   - return 0 on success, non-zero on error; ssad_last_error() returns a message for
 *     the calling thread.  Never aborts.
 *   - activations are NHWC fp32 inside the library; conv weights are OHWI fp32
 *     ([Cout][KH][KW][Cin]); images enter as NCHW fp32 exactly as the reference's
 *     Dataset emits them (src/self_supervised/datasets.py:394).
 */
#ifndef SSAD_H
#define SSAD_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SSAD_VERSION 100

int ssad_version(void);
const char* ssad_last_error(void);

/* ---- weight repacking (checkpoint tensors keep the reference's OIHW shapes, SURVEY s.5) ---- */
/* OIHW -> OHWI.  Linear weights [out][in] are already "OHWI" with KH=KW=1. */
int ssad_repack_oihw_to_ohwi(const float* w_oihw, float* w_ohwi, int O, int I, int KH, int KW, void* stream);
int ssad_repack_ohwi_to_oihw(const float* w_ohwi, float* w_oihw, int O, int I, int KH, int KW, void* stream);
/* conv1 7x7 OIHW [64][3][7][7] -> MFMA K-order [168][64] (kx padded 7->8 with zeros). */
int ssad_pack_stem_weight(const float* w_oihw, float* wk, void* stream);
/* The same pack from an OHWI filter [64][7][7][3]: how the training step's parameter arena holds conv1 (models.py:224 under trainer.fit);
 * spares the step an OIHW copy of the weight per iteration (round 6). */
int ssad_pack_stem_weight_ohwi(const float* w_ohwi, float* wk, void* stream);

/* ---- forward kernels ---- */
/* Replaces: extract_patches (src/self_supervised/functional.py:77-82) + reshape
 * (src/self_supervised/models.py:212-214) + F.interpolate(x, 64, 'nearest') (models.py:217-219)
 * + resnet conv1/bn1/relu (models.py:224; torchvision resnet18 stem), fused: the patch window and
 * the nearest resize are applied in the loader, nothing is materialised.
 *   img      : [B][3][H][W] NCHW fp32
 *   patch_dim/patch_stride : sliding window (32, 8); patch_dim = 0 -> whole image is one sample
 *   Hv, Wv   : size after the nearest resize (== window size when no resize happens)
 *   wk       : ssad_pack_stem_weight output
 *   scale/shift : per-channel affine applied to the conv output (eval-mode BN folded); NULL -> raw conv
 *   out      : [Nsamp][Ho][Wo][64] NHWC, Ho = (Hv-1)/2+1.  Nsamp = B * patches per image.
 *   hwnc     : 1 -> write the position-major layout [Ho][Wo][Nsamp][64] (patch-scoring trunk, see
 *              ssad_conv_igemm_fwd_hwnc); the same flag selects the layout in ssad_maxpool3x3s2_fwd / ssad_gap_fwd.
 */
int ssad_stem_fwd(const float* img, int B, int H, int W, int patch_dim, int patch_stride, int Hv, int Wv,
                  const float* wk, const float* scale, const float* shift, int relu, int hwnc, float* out, void* stream);
/* The same conv1 in training (no patch window, no affine): raw z plus the train-mode statistics of bn1 in one pass
 * (models.py:224 under trainer.fit).  workspace: ssad_stem_stats_rows() * 128 doubles (one [2][64] row per workgroup). */
int ssad_stem_stats_rows(void);
int ssad_stem_fwd_stats(const float* img, int B, int H, int W, int Hv, int Wv, const float* wk, float* out, float eps,
                        float momentum, float* mean, float* invstd, float* running_mean, float* running_var, double* workspace,
                        void* stream);

/* Patch-scoring specialisation of the stem (32x32 windows, exact 2x nearest upsample): the same call sites as
 * ssad_stem_fwd + ssad_maxpool3x3s2_fwd fused into one kernel.  conv7x7/2 over the upsampled window is evaluated as
 * the equivalent 4x4 stride-1 conv over the 32x32 source with pre-summed weights (wf = ssad_pack_stem_weight_folded),
 * BN+ReLU+max-pool are applied in LDS; out = [Nsamp][16][16][64] (or [16][16][Nsamp][64] when hwnc). */
int ssad_pack_stem_weight_folded(const float* w_oihw, float* wf, void* stream);
int ssad_stem_patch_pool_fwd(const float* img, int B, int H, int W, int patch_stride, const float* wf, const float* scale,
                             const float* shift, int hwnc, float* out, void* stream);
/* The same without the pooled positions skip_lo <= py, px <= skip_hi of every patch (neither pooled nor stored): with layer1 shared between
 * overlapping patches the first ring conv (ssad_conv_igemm_fwd_hwnc_ring) reads the pooled map within one position of the outputs it
 * computes -- the interior is read by nobody. */
int ssad_stem_patch_pool_fwd_ring(const float* img, int B, int H, int W, int patch_stride, const float* wf, const float* scale,
                                  const float* shift, int hwnc, int skip_lo, int skip_hi, float* out, void* stream);
/* Only the BORDER of that pooled map -- rows / columns 0, 1 and 15 of every patch, the positions where the patch's own zero padding makes
 * it differ from the per-image pooled map -- written position-major [16][16][Nsamp][64]; the other positions are left untouched
 * (ssad_patch_gather_hwnc_band copies rows / columns 2-3 and 13-14 from the per-image map; nobody reads the rest).  Values bit-identical
 * to ssad_stem_patch_pool_fwd at the positions written. */
int ssad_stem_patch_border_fwd(const float* img, int B, int H, int W, int patch_stride, const float* wf, const float* scale,
                               const float* shift, float* out, void* stream);

/* Replaces nn.MaxPool2d(3, 2, 1) of the torchvision stem (models.py:224).  NHWC, or [H][W][N][C] when hwnc. */
int ssad_maxpool3x3s2_fwd(const float* in, float* out, int64_t N, int H, int W, int C, int hwnc, void* stream);

/* Replaces every nn.Conv2d(3x3 / 1x1, bias=False) + eval BatchNorm2d + residual add + ReLU of the
 * BasicBlocks (models.py:224), and every nn.Linear (+BatchNorm1d, +ReLU) of concatenator /
 * latent_space / classifier (models.py:247-249) with H=W=KH=KW=1.  Implicit GEMM on
 * v_mfma_f32_32x32x2_f32: out[m][co] = act( (sum_k in[m,k] * w[co,k]) * scale[co] + shift[co] + residual[m][co] ).
 * Requires Cin % 32 == 0.  scale/shift/residual may be NULL.
 */
int ssad_conv_igemm_fwd(const float* in, const float* w_ohwi, float* out, const float* scale, const float* shift,
                        const float* residual, int relu, int64_t N, int H, int W, int Cin, int Cout, int KH, int KW,
                        int stride, int pad, void* stream);

/* Same contraction with every activation tensor (in, out, residual) stored position-major, [H][W][N][C]: the layout
 * of the patch-scoring trunk (thousands of patches with 16x16 .. 2x2 maps).  A workgroup's 128 rows are 128 patches
 * at one output position: contiguous in HBM for every filter tap, and taps that fall into the zero padding are
 * skipped as whole K-steps (exact: only x*0 products are dropped). */
int ssad_conv_igemm_fwd_hwnc(const float* in, const float* w_ohwi, float* out, const float* scale, const float* shift,
                             const float* residual, int relu, int64_t N, int H, int W, int Cin, int Cout, int KH, int KW,
                             int stride, int pad, void* stream);

/* Round 6: the layer1 convolutions of the patch-scoring pass without the arithmetic that overlapping patches share.
 * PeraNet.forward in patch mode (models.py:211-224) runs resnet layer1 on 841 windows of 32 x 32 pixels at stride 8 per image
 * (functional.py:77-82); away from a window's own zero-padded border a conv output is the same sum over the same pixels in every
 * window covering them, i.e. the value of the conv run ONCE over the whole image's map.  ssad_conv_igemm_fwd_hwnc_ring computes only
 * the output positions outside the square skip_lo <= oy, ox <= skip_hi (position-major tensors as ssad_conv_igemm_fwd_hwnc; the
 * positions inside are not touched), ssad_patch_gather_hwnc copies the positions lo <= u, v <= hi of every patch from the per-image
 * dense map: out[u][v][n][:] = dense[b][shift * pr + u][shift * pc + v][:], n = (b * prow + pr) * pcol + pc, dense NHWC
 * [B][Hd][Wd][C], out [H][W][N][C].  Exact: no product is approximated, only not repeated. */
int ssad_conv_igemm_fwd_hwnc_ring(const float* in, const float* w_ohwi, float* out, const float* scale, const float* shift,
                                  const float* residual, int relu, int64_t N, int H, int W, int Cin, int Cout, int KH, int KW,
                                  int stride, int pad, int skip_lo, int skip_hi, void* stream);
int ssad_patch_gather_hwnc(const float* dense, float* out, int64_t B, int prow, int pcol, int shift, int Hd, int Wd, int C,
                           int H, int W, int lo, int hi, void* stream);
/* The same copy without the inner square ilo <= u, v <= ihi (ilo > ihi: none): the ring conv that follows reads its input within one
 * position of the outputs it computes, the deep interior of an intermediate layer1 map is read by nobody. */
int ssad_patch_gather_hwnc_band(const float* dense, float* out, int64_t B, int prow, int pcol, int shift, int Hd, int Wd, int C,
                                int H, int W, int lo, int hi, int ilo, int ihi, void* stream);

/* Which exact-fp32 instantiation an implicit-GEMM entry point gives a problem: BM * 100000 + BN * 100 + BK of the workgroup
 * tile, negated when its rows are position-major.  mode: 0 ssad_conv_igemm_fwd, 1 ssad_conv_igemm_fwd_hwnc,
 * 2 ssad_conv_igemm_fwd_hwnc_ring, 3 ssad_conv_igemm_fwd_stats, 4 ssad_conv_igemm_dgrad / _dgrad_masked.  The arguments are
 * always the forward conv's (mode 4: x [N][H][W][Cin] -> y [N][Ho][Wo][Cout] at stride 1 or 2, the gradient flowing back to x).
 * Host-only (no GPU needed).  Measurement and test aid (bench.py names the instantiations its roofline figure sums over;
 * tests/test_igemm_tile_table.py pins the selection); no reference counterpart. */
int ssad_conv_igemm_tile(int64_t N, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad, int mode);
/* The same choice as the IgemmTile value of csrc/conv_igemm.hip (0 .. 12), + 100 when the rows are position-major: tells apart
 * the instantiations that share a BM / BN / BK (single- and double-buffered, four-wave 256 x 128). */
int ssad_conv_igemm_tile_id(int64_t N, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad, int mode);

/* Replaces F.adaptive_avg_pool2d(., (1,1)) + flatten + torch.cat (models.py:227-245):
 * out[n*out_stride + out_offset + c] = mean over HW of in[n][hw][c]. */
int ssad_gap_fwd(const float* in, float* out, int64_t N, int HW, int C, int out_stride, int out_offset, int hwnc,
                 void* stream);

/* ---- scoring ---- */
/* Replaces sklearn NearestNeighbors(metric='cosine').kneighbors + torch.mean (models.py:352-370).
 * l2norm: out[i] = x[i] / ||x[i]||, a row whose fp32 sum of squares is exactly 0 divided by 1 (sklearn's normalize).  knn3: given sim[Nq][Nb] = qn . bn, writes mean of the 3 smallest
 * clip(1 - sim, 0, 2) per row. */
int ssad_l2_normalize_rows(const float* x, float* out, int64_t N, int D, void* stream);
int ssad_cosine_knn_mean(const float* sim, float* out, int64_t Nq, int Nb, int k, void* stream);

/* Replaces tools.upsample (src/self_supervised/tools.py:394-399): relu(gaussian_blur(k, sigma=0.15k+0.35,
 * reflect)) then bilinear (align_corners=False) to target x target.  maps [n][h][w] -> out [n][target][target]. */
int ssad_blur_relu_bilinear(const float* maps, float* out, int n, int h, int w, int ksize, int target, void* stream);

/* Grad-CAM contraction (src/self_supervised/gradcam.py:39-43): out[b][pos] = sum_k alpha[b][k] * act[b][pos][k] for the
 * NHWC layer4 activations act [B][HW][C]; alpha rows are alpha_stride floats apart (a slice of the pooled-feature
 * gradient).  ReLU + the bilinear resize to the input size are ssad_blur_relu_bilinear with ksize = 1. */
int ssad_gradcam_map(const float* act, const float* alpha, float* out, int64_t B, int HW, int C, int alpha_stride,
                     void* stream);

/* Replaces sklearn roc_curve + auc as called for pixel / image AUROC (src/self_supervised/metrics.py:49-56,
 * src/self_supervised/tools.py:76-98) when the scores are already on the GPU: radix sort + tie-aware rank sum, exact
 * integer counts reduced in fp64.  labels: uint8, non-zero = anomalous.  out[0] = AUROC, out[1] = #positives. */
int64_t ssad_auroc_workspace(int64_t n);
int ssad_auroc(const float* scores, const uint8_t* labels, int64_t n, void* workspace, int64_t workspace_bytes, double* out,
               void* stream);

/* ---- training step (forward in train mode, backward, update) ---- */
/* Replaces autograd's conv2d/linear input-gradient (loss.backward() inside pl.Trainer.fit, tools.py:270,:303).
 * w_flipT = ssad_flip_transpose_weight(w_ohwi).  dx = dgrad(dy) (+ residual).  Cout % 32 == 0. */
int ssad_flip_transpose_weight(const float* w_ohwi, float* out, int O, int I, int KH, int KW, void* stream);
/* ... for n filters of one arena, one launch per 32 of them: desc[k] = {src offset, dst offset, O, I, KH, KW} (host memory). */
int ssad_flip_transpose_batch(const float* src, float* dst, const int64_t* desc, int n, void* stream);
int ssad_conv_igemm_dgrad(const float* dy, const float* w_flipT, float* dx, const float* residual, int64_t N, int Hy, int Wy,
                          int Cout, int Hx, int Wx, int Cin, int KH, int KW, int stride, int pad, void* stream);
/* Split-bf16 ("bf16x3") forms of the forward / position-major forward (hwnc != 0) and dgrad contractions: fp32 tensors in
 * and out; every operand x is staged as hi = bf16(x), lo = bf16(x - hi) and every product is hi*hi + hi*lo + lo*hi on
 * the bf16 matrix cores with fp32 accumulation -- ~2^-17 relative error per product at 3/16 of the fp32-MFMA time.
 * Opt-in (SSAD_MATH=bf16x3 / Trainer(precision="bf16x3")); held to the same 1e-4 parity bar as the exact fp32 path. */
int ssad_conv_igemm_fwd_x3(const float* in, const float* w_ohwi, float* out, const float* scale, const float* shift,
                           const float* residual, int relu, int64_t N, int H, int W, int Cin, int Cout, int KH, int KW,
                           int stride, int pad, int hwnc, void* stream);
int ssad_conv_igemm_dgrad_x3(const float* dy, const float* w_flipT, float* dx, const float* residual, int64_t N, int Hy,
                             int Wy, int Cout, int Hx, int Wx, int Cin, int KH, int KW, int stride, int pad, void* stream);
/* Three-way split ("bf16x6"): x = hi + mid + lo (24 significant bits) and the six products of weight >= 2^-18; what is
 * dropped is ~2^-25 of each product, i.e. fp32-faithful products at 6/16 of the fp32-MFMA time. */
int ssad_conv_igemm_fwd_x6(const float* in, const float* w_ohwi, float* out, const float* scale, const float* shift,
                           const float* residual, int relu, int64_t N, int H, int W, int Cin, int Cout, int KH, int KW,
                           int stride, int pad, int hwnc, void* stream);
int ssad_conv_igemm_dgrad_x6(const float* dy, const float* w_flipT, float* dx, const float* residual, int64_t N, int Hy,
                             int Wy, int Cout, int Hx, int Wx, int Cin, int KH, int KW, int stride, int pad, void* stream);
/* BatchNorm over a few hundred rows (the BatchNorm1d layers of the projection head on a training batch, models.py:65-95) in one
 * launch each way: statistics + running-statistics update + apply (+ ReLU) forward; the two column sums, their use and optionally
 * the bias gradient of the Linear in front (dbias = column sums of dz) backward.  zmask_beta != NULL: the layer's ReLU mask is
 * recomputed from z (no residual in between).  ssad_bn_small_ok(R, C): R <= 512 rows, C a multiple of 32. */
int ssad_bn_small_ok(int64_t R, int C);
int ssad_bn_small_fwd(const float* z, const float* gamma, const float* beta, float* y, float* mean, float* invstd,
                      float* running_mean, float* running_var, int64_t R, int C, float eps, float momentum, int relu, void* stream);
int ssad_bn_small_bwd(const float* dy, const float* z, const float* mean, const float* invstd, const float* gamma,
                      const float* zmask_beta, float* dbeta, float* dgamma, float* dbias, float* dz, int64_t R, int C, void* stream);
/* Linear layers over a training batch's few rows (the projection head and classifier, models.py:65-99, :247-252): 1 x 1 layers on
 * 1 x 1 maps with N <= ssad_linear_small_max_rows() rows are served by a dedicated kernel (contraction dealt over the waves of a
 * 32 x 32 output tile) inside ssad_conv_igemm_fwd / _fwd_stats / _dgrad -- those then accept any Cin (Cout for dgrad) % 4 == 0 --
 * and their weight gradient by ssad_linear_wgrad_small: dw[Cout][Cin] (+)= dy[M][Cout]^T x[M][Cin], one launch, no slab.
 * SSAD_LINEAR_SMALL=0 in the environment switches the range off (max_rows 0). */
int ssad_linear_small_max_rows(void);
int ssad_linear_wgrad_small(const float* dy, const float* x, float* dw, int64_t M, int Cin, int Cout, int accumulate, void* stream);
/* the same with its operands rounded to bf16 (round = 1) / fp16 (round = 2) while loaded: the precision-16 step's linear layers */
int ssad_linear_wgrad_small_r(const float* dy, const float* x, float* dw, int64_t M, int Cin, int Cout, int accumulate, int round,
                              void* stream);
/* Replaces autograd's conv2d/linear weight-gradient.  Two launches: partial tiles per pixel split into
 * slab[splits][Cout][KH*KW*Cin], then a fixed-order sum written as OIHW (to_oihw=1, checkpoint layout) or OHWI.
 * Guard convention (round 5): wherever an entry point reads a SECOND tensor over extents it derives from the first one's (dy from
 * x's N, H, W and the filter geometry; dz from the image size; the pooled gradient from z's size), the caller also states how many
 * elements that second buffer holds (`dy_elems`, `dz_elems`, `dpool_elems`); a count that does not match the derived extents is an
 * error return, not an out-of-bounds read. */
int ssad_wgrad_splits(int64_t M, int Cin, int Cout, int KH, int KW);
int ssad_wgrad_splits_bf16(int64_t M, int Cin, int Cout, int KH, int KW);   /* for ssad_conv_wgrad_bf16 / _x3 */
int ssad_conv_wgrad(const float* dy, const float* x, float* slab, int splits, int64_t N, int H, int W, int Cin, int Cout,
                    int KH, int KW, int stride, int pad, int64_t dy_elems, void* stream);
int ssad_conv_wgrad_x3(const float* dy, const float* x, float* slab, int splits, int64_t N, int H, int W, int Cin, int Cout,
                       int KH, int KW, int stride, int pad, int64_t dy_elems, void* stream);   /* split-bf16 products, see ssad_conv_igemm_fwd_x3 */
int ssad_conv_wgrad_x6(const float* dy, const float* x, float* slab, int splits, int64_t N, int H, int W, int Cin, int Cout,
                       int KH, int KW, int stride, int pad, int64_t dy_elems, void* stream);   /* three-way split, see ssad_conv_igemm_fwd_x6 */
int ssad_wgrad_reduce(const float* slab, float* dw, int splits, int Cout, int Kpad, int KH, int KW, int Cin, int to_oihw,
                      int accumulate, void* stream);
/* Several such reductions in ONE launch (round 6): desc[6 k ..] = slab pointer, output pointer (as integers), splits, Cout, Kpad,
 * Kreal = KH * KW * Cin.  Nothing on the backward pass's critical path reads a weight gradient, so the training step collects the
 * reductions of its weight-gradient kernels and runs them where the gradients are first needed (optimizer / a gradient bucket).
 * Same order of additions per output as ssad_wgrad_reduce: bit-identical.  OHWI outputs, no accumulation; Kreal % 4 == 0, Kpad % 4 == 0,
 * 16-byte aligned pointers.  Same autograd nodes as ssad_conv_wgrad (Conv2d weight gradients under trainer.fit, models.py:256-277). */
int ssad_wgrad_reduce_batch(const int64_t* desc, int n, void* stream);
/* The instantiation a weight-gradient launch of a given path runs -- the launchers take their template arguments from this same
 * function.  Host-only (no GPU needed); test aid (tests/test_wgrad_path_table.py pins the selection), no reference counterpart.
 *   SSAD_WGRAD_GENERIC  ssad_conv_wgrad and its 16-bit / split-bf16 forms: the channel tile BT, 64 or 128
 *   SSAD_WGRAD_HALO     ssad_conv_wgrad3x3_halo (stride 1) / ssad_conv_wgrad3x3s2_halo (stride 2)   the output-pixel tile,
 *   SSAD_WGRAD_HALO16   ssad_conv_wgrad3x3_halo16(_h) (stride 1)                                     TH * 100 + TW
 *   SSAD_WGRAD_G16      ssad_conv_wgrad3x3_g16_h (stride 1 or 2)                                     (416 = 4 x 16, ...)
 *   SSAD_WGRAD_STEM     ssad_stem_wgrad (dz_half 0) / ssad_stem_wgrad_h (dz_half 1): 0 fp32 dz, 1 half dz on the fp32 MFMAs,
 *                       2 fp16 operands
 * Wo: width of dz (the conv's OUTPUT).  -1 for an unknown path. */
#define SSAD_WGRAD_GENERIC 0
#define SSAD_WGRAD_HALO 1
#define SSAD_WGRAD_HALO16 2
#define SSAD_WGRAD_G16 3
#define SSAD_WGRAD_STEM 4
int ssad_wgrad_variant_id(int path, int Wo, int Cin, int Cout, int stride, int dz_half);
/* bf16-operand forms of the three MFMA entry points above (fp32 tensors in HBM; operands rounded to bf16 while staging,
 * fp32 accumulate; v_mfma_f32_32x32x16_bf16).  This is what torch.autocast does to the same Conv2d / Linear call sites
 * under the reference's pl.Trainer(precision=16) (src/self_supervised/tools.py:263, :296). */
int ssad_conv_igemm_fwd_bf16(const float* in, const float* w_ohwi, float* out, const float* scale, const float* shift,
                             const float* residual, int relu, int64_t N, int H, int W, int Cin, int Cout, int KH, int KW,
                             int stride, int pad, void* stream);
int ssad_conv_igemm_dgrad_bf16(const float* dy, const float* w_flipT, float* dx, const float* residual, int64_t N, int Hy,
                               int Wy, int Cout, int Hx, int Wx, int Cin, int KH, int KW, int stride, int pad, void* stream);
int ssad_conv_wgrad_bf16(const float* dy, const float* x, float* slab, int splits, int64_t N, int H, int W, int Cin, int Cout,
                         int KH, int KW, int stride, int pad, int64_t dy_elems, void* stream);
/* Halo-tile direct convolution for the 64 -> 64 channel 3x3 / stride 1 / pad 1 layers (torchvision BasicBlock conv3x3 of
 * ResNet-18 layer1, models.py:224 of the reference under trainer.fit, and their input gradients -- call it with
 * ssad_flip_transpose_weight(w) and dy): out = conv(T(in)) (+ residual), NHWC fp32, OHWI weights, exact fp32 MFMA.
 * res_mask (optional, with residual): nibble mask of ssad_bn_apply_fwd_mask -- only the masked elements of the residual are added.
 * T = identity, or relu((x - tr_mean) * tr_invstd * tr_gamma + tr_beta) per input channel (the train-mode BatchNorm + ReLU of
 * the producing layer, applied while the input tile is staged); `emit` (optional) receives T(in).  stats_ws != NULL: also
 * the train-mode BatchNorm statistics of the output (ssad_conv3x3_c64_stats_rows(N, H, W) * 128 doubles of workspace),
 * mean / invstd / running statistics as ssad_conv_igemm_fwd_stats produces them. */
int64_t ssad_conv3x3_c64_stats_rows(int64_t N, int H, int W);
int ssad_conv3x3_c64(const float* in, const float* w_ohwi, float* out, const float* residual, const uint8_t* res_mask, const float* tr_mean,
                     const float* tr_invstd, const float* tr_gamma, const float* tr_beta, float* emit, int64_t N, int H, int W,
                     double* stats_ws, float eps, float momentum, float* mean, float* invstd, float* running_mean,
                     float* running_var, void* stream);
/* The same with op = 1 / 2: bf16 / fp16 OPERANDS (fp32 tensors, rounded while staged; fp32 accumulation, statistics, transform and
 * emit) -- the layer1 convolutions of the reference's fp16-autocast training (pl.Trainer(precision=16), tools.py:263); op = 0 is
 * ssad_conv3x3_c64. */
int ssad_conv3x3_c64_op(const float* in, const float* w_ohwi, float* out, const float* residual, const uint8_t* res_mask,
                        const float* tr_mean, const float* tr_invstd, const float* tr_gamma, const float* tr_beta, float* emit, int64_t N,
                        int H, int W, double* stats_ws, float eps, float momentum, float* mean, float* invstd, float* running_mean,
                        float* running_var, int op, void* stream);
/* Inference form of the halo-tile convolution (frozen BatchNorm folded into scale / shift):
 * out = act(conv3x3(in) * scale[co] + shift[co] + residual), 64 -> 64 channels, stride 1, pad 1, exact fp32 MFMA.
 * in_hwnc / out_hwnc / res_hwnc != 0: the input / the output / the residual is position-major [H][W][N][64] (the
 * patch-scoring trunk's layout, see ssad_conv_igemm_fwd_hwnc), otherwise NHWC.  Replaces ssad_conv_igemm_fwd(_hwnc) for the four layer1
 * convolutions of PeraNet.forward in eval mode (torchvision BasicBlock, models.py:224 of the reference). */
int ssad_conv3x3_c64_eval(const float* in, const float* w_ohwi, float* out, const float* scale, const float* shift,
                          const float* residual, int relu, int64_t N, int H, int W, int in_hwnc, int out_hwnc, int res_hwnc,
                          void* stream);
/* The launch geometry of the three 3 x 3 / stride 1 / pad 1 kernels -- the launchers take their values from the same functions.
 * Host-only (no GPU needed); test aid (tests/test_conv3x3_table.py pins it), no reference counterpart.
 *   SSAD_CONV3X3_C64  ssad_conv3x3_c64 / _op / _h / _eval (Cin = Cout = 64; one workgroup per 8 x 16 tile)
 *   SSAD_CONV3X3_H    ssad_conv3x3_h
 *   SSAD_CONV3X3_W    ssad_conv3x3_hw (is_float 0) / ssad_conv3x3_fw, _fw_eval (is_float 1), WITHOUT the minimum-work rule of
 *                     ssad_conv3x3_hw_ok / _fw_ok (the entry points have none)
 * out[0] instantiation: C64 816; H: bn * 10 + tw8 (bn = channels per workgroup, 64 / 128; tw8 = two 8-row strips of a map up to 8
 *        wide per tile); W: wn * 10000 + tw8 * 1000 + twp * 100 + channels per input chunk (wn = 64-channel wave columns; tw8 = four
 *        8 x 8 maps per tile; twp = two 16 x 16 maps per tile)
 * out[1] ntiles   out[2] gx (workgroups per channel slab = rows of the statistics workspace)   out[3] gy (channel slabs)
 * out[4] input chunks per tile   out[5] maps present in the last tile   out[6] most tiles one workgroup walks, ceil(ntiles / gx)
 * out[7] maps per tile
 * Returns non-zero (out untouched) for a path or a shape the entry point refuses. */
#define SSAD_CONV3X3_C64 0
#define SSAD_CONV3X3_H 1
#define SSAD_CONV3X3_W 2
int ssad_conv3x3_geometry(int path, int64_t N, int H, int W, int Cin, int Cout, int is_float, int64_t* out);
/* Weight gradient of the 3x3 / stride 1 / pad 1 convolutions (Cin, Cout multiples of 64) as a halo-tile kernel: a workgroup
 * owns a 64 x 64 (co, ci) block for all nine taps and walks over pixel tiles (csrc/wgrad_halo.hip).  Same contract as
 * ssad_conv_wgrad: slab[splits][Cout][9 * Cin] with splits = ssad_wgrad3x3_halo_splits(...), then ssad_wgrad_reduce. */
int ssad_wgrad3x3_halo_ok(int Cin, int Cout, int KH, int KW, int stride, int pad);   /* 0 no, 1 stride-1 form, 2 stride-2 form */
int ssad_wgrad3x3_halo_splits(int64_t N, int H, int W, int Cin, int Cout);            /* H, W: size of dz (the conv's OUTPUT) */
int ssad_conv_wgrad3x3_halo(const float* dz, const float* x, float* slab, int splits, int64_t N, int H, int W, int Cin, int Cout,
                            int64_t dz_elems, void* stream);
/* 3x3 / stride 2 / pad 1 (the first convolution of layer2-4): dz [N][Ho][Wo][Cout], x [N][H][W][Cin], Ho = (H - 1) / 2 + 1. */
int ssad_conv_wgrad3x3s2_halo(const float* dz, const float* x, float* slab, int splits, int64_t N, int Ho, int Wo, int H, int W,
                              int Cin, int Cout, int64_t dz_elems, void* stream);
/* Stem conv 7x7 / 2 of the precision-16 training step (csrc/stem16.hip): fp16 (f16 != 0) or bf16 operands, fp32 accumulation; the
 * 16-bit counterpart of ssad_stem_fwd_stats for whole images -- resnet.conv1 + bn1 statistics under fp16 autocast
 * (pl.Trainer(precision=16), src/self_supervised/tools.py:263; models.py:224).  wk16: 14 * 64 * 16 halves from ssad_pack_stem_weight16;
 * workspace: ssad_stem_stats_rows() * 128 doubles. */
int ssad_pack_stem_weight16(const float* w_oihw, void* wk16, int f16, void* stream);
int ssad_pack_stem_weight16_ohwi(const float* w_ohwi, void* wk16, int f16, void* stream);   /* OHWI source, as ssad_pack_stem_weight_ohwi */
int ssad_stem_fwd_stats16(const float* img, int B, int H, int W, const void* wk16, float* out, float eps, float momentum, float* mean,
                          float* invstd, float* running_mean, float* running_var, double* workspace, int f16, void* stream);
/* The same halo-tile weight gradient with 16-bit OPERANDS (fp32 tensors in memory, rounded to fp16 -- f16 != 0 -- or bf16 while
 * staged, fp32 accumulation; csrc/wgrad_halo16.hip): the conv2d weight gradient of the reference's fp16-autocast training
 * (pl.Trainer(precision=16), src/self_supervised/tools.py:263, :270, :303) for the 3 x 3 / stride 1 / pad 1 layers.  Same slab contract:
 * splits = ssad_wgrad3x3_halo16_splits(...), then ssad_wgrad_reduce. */
int ssad_wgrad3x3_halo16_ok(int Cin, int Cout, int KH, int KW, int stride, int pad);
int ssad_wgrad3x3_halo16_splits(int64_t N, int H, int W, int Cin, int Cout);
int ssad_conv_wgrad3x3_halo16(const float* dz, const float* x, float* slab, int splits, int64_t N, int H, int W, int Cin, int Cout,
                              int f16, int64_t dz_elems, void* stream);
/* fp16-operand forms: the reference trains under fp16 autocast (pl.Trainer(precision=16), src/self_supervised/tools.py:263,
 * :296), i.e. its Conv2d / Linear products take fp16 operands and accumulate in fp32.  Same contract as the _bf16 forms
 * with v_mfma_f32_32x32x16_f16 (11-bit significands); the slab of ssad_conv_wgrad_f16 is sized by ssad_wgrad_splits_bf16. */
int ssad_conv_igemm_fwd_f16(const float* in, const float* w_ohwi, float* out, const float* scale, const float* shift,
                            const float* residual, int relu, int64_t N, int H, int W, int Cin, int Cout, int KH, int KW,
                            int stride, int pad, void* stream);
int ssad_conv_igemm_dgrad_f16(const float* dy, const float* w_flipT, float* dx, const float* residual, int64_t N, int Hy,
                              int Wy, int Cout, int Hx, int Wx, int Cin, int KH, int KW, int stride, int pad, void* stream);
int ssad_conv_wgrad_f16(const float* dy, const float* x, float* slab, int splits, int64_t N, int H, int W, int Cin, int Cout,
                        int KH, int KW, int stride, int pad, int64_t dy_elems, void* stream);
/* Stem in training: im2col rows of 160 floats (147 taps + zero pad, nearest resize fused) so that conv1 forward and
 * its weight gradient run on the generic MFMA kernels.  Replaces conv1 of torchvision resnet18 under autograd. */
int ssad_stem_im2col(const float* img, float* col, int64_t B, int H, int W, int Hv, int Wv, void* stream);
/* Weight gradient of resnet conv1 (7x7/2, 3 -> 64; autograd node of models.py:224 inside trainer.fit) straight from the
 * NCHW image -- no im2col buffer.  dz NHWC [B][Ho][Wo][64] with Ho, Wo as ssad_stem_fwd computes them (images below
 * 64x64 go through the same nearest resize).  dw receives 64*7*7*3 floats, OHWI or (to_oihw) OIHW, optionally
 * accumulated.  workspace: ssad_stem_wgrad_workspace(B, H, W) floats (per-workgroup slabs, summed in a fixed order). */
int64_t ssad_stem_wgrad_workspace(int B, int H, int W);
int ssad_stem_wgrad_splits(int B, int H, int W);     /* slabs in that workspace (= the reduction's split count); host-only */
int ssad_stem_wgrad(const float* img, const float* dz, float* dw, int B, int H, int W, int64_t dz_elems, int to_oihw,
                    int accumulate, float* workspace, void* stream);
int ssad_pack_stem_weight_2d(const float* w_oihw, float* out, void* stream);
/* Replaces nn.BatchNorm2d / nn.BatchNorm1d in training mode (models.py:65-95 + torchvision BasicBlock):
 * batch statistics over R rows (biased variance for normalisation, unbiased for running_var, momentum),
 * y = (z-mean)*invstd*gamma+beta (+residual)(ReLU), and the matching backward.  workspace: doubles, see
 * ssad_colreduce_workspace. */
int64_t ssad_colreduce_workspace(int64_t R, int C);
int ssad_bn_stats(const float* z, int64_t R, int C, float eps, float momentum, float* mean, float* invstd,
                  float* running_mean, float* running_var, double* workspace, void* stream);
/* Conv2d (bias-free, as in every BasicBlock: torchvision resnet.py conv3x3/conv1x1) + the batch statistics of the
 * train-mode BatchNorm2d that follows it (models.py:224-243 under trainer.fit) in one pass: the conv kernel leaves
 * per-workgroup double-precision column sums in `workspace` (ssad_conv_stats_workspace(N, Ho, Wo, Cout) doubles), a
 * finalize launch produces mean / invstd and updates the running statistics exactly as ssad_bn_stats does.
 * `out` receives the raw convolution z (NHWC).  bf16: operand mode, 0 fp32, 1 bf16, 2 fp16, 3 / 6 split-bf16. */
int64_t ssad_conv_stats_workspace(int64_t N, int Ho, int Wo, int Cout);
int ssad_conv_igemm_fwd_stats(const float* in, const float* w_ohwi, float* out, int64_t N, int H, int W, int Cin, int Cout,
                              int KH, int KW, int stride, int pad, int bf16, float eps, float momentum, float* mean,
                              float* invstd, float* running_mean, float* running_var, double* workspace, void* stream);
int ssad_bn_apply_fwd(const float* z, const float* mean, const float* invstd, const float* gamma, const float* beta,
                      const float* residual, float* y, int64_t R, int C, int relu, void* stream);
int ssad_bn_bwd_reduce(const float* dy, const float* yact, const float* z, const float* mean, const float* invstd,
                       float* dbeta, float* dgamma, int64_t R, int C, double* workspace, void* stream);
int ssad_bn_apply_bwd(const float* dy, const float* yact, const float* z, const float* mean, const float* invstd,
                      const float* gamma, const float* dbeta, const float* dgamma, float* dz, float* dres, int64_t R, int C,
                      int eval_mode, void* stream);
/* Residual blocks without the saved-activation reads: ssad_bn_apply_fwd_mask also writes the final ReLU's active set as a
 * nibble mask (one byte per channel quad, bit k = channel 4q+k positive: 1/16 of the activation's bytes); the backward
 * reductions / apply take g = dy * mask from it (mask4 NULL: no ReLU), and the gradient of the identity branch -- dy under the
 * same mask -- is applied by the consumer (ssad_conv_igemm_dgrad_masked, ssad_conv3x3_c64 res_mask) instead of being stored.
 * Replaces the same autograd nodes as ssad_bn_apply_fwd / _bwd_reduce / _apply_bwd (torchvision BasicBlock bn2 + add + relu). */
int ssad_bn_apply_fwd_mask(const float* z, const float* mean, const float* invstd, const float* gamma, const float* beta,
                           const float* residual, float* y, uint8_t* mask4, int64_t R, int C, int relu, void* stream);
int ssad_bn_bwd_reduce_mask(const float* dy, const uint8_t* mask4, const float* z, const float* mean, const float* invstd,
                            float* dbeta, float* dgamma, int64_t R, int C, double* workspace, void* stream);
int ssad_bn_apply_bwd_mask(const float* dy, const uint8_t* mask4, const float* z, const float* mean, const float* invstd,
                           const float* gamma, const float* dbeta, const float* dgamma, float* dz, int64_t R, int C, void* stream);
/* The same three over half tensors (the precision-16 step, round 6): a lane's 8 channels take two mask bytes; the mask is that of the
 * STORED half activation.  Same autograd nodes under pl.Trainer(precision=16) (tools.py:263). */
int ssad_bn_apply_fwd_mask_h(const void* z, const float* mean, const float* invstd, const float* gamma, const float* beta,
                             const void* residual, void* y, uint8_t* mask4, int64_t R, int C, int relu, void* stream);
int ssad_bn_bwd_reduce_mask_h(const void* dy, const uint8_t* mask4, const void* z, const float* mean, const float* invstd,
                              float* dbeta, float* dgamma, int64_t R, int C, double* workspace, void* stream);
int ssad_bn_apply_bwd_mask_h(const void* dy, const uint8_t* mask4, const void* z, const float* mean, const float* invstd,
                             const float* gamma, const float* dbeta, const float* dgamma, void* dz, int64_t R, int C, void* stream);
int ssad_conv_igemm_dgrad_masked(const float* dy, const float* w_flipT, float* dx, const float* residual, const uint8_t* res_mask,
                                 int64_t N, int Hy, int Wy, int Cout, int Hx, int Wx, int Cin, int KH, int KW, int stride, int pad,
                                 void* stream);
/* The same two calls for a BatchNorm + ReLU with NO residual in between (conv1 of a BasicBlock, the stem, the head's
 * Linear+BN+ReLU): the ReLU mask is recomputed as (z - mean) * invstd * gamma + beta > 0 -- the expression the forward
 * evaluated -- so the saved activation is not read again. */
int ssad_bn_bwd_reduce_zmask(const float* dy, const float* z, const float* mean, const float* invstd, const float* gamma,
                             const float* beta, float* dbeta, float* dgamma, int64_t R, int C, double* workspace,
                             void* stream);
int ssad_bn_apply_bwd_zmask(const float* dy, const float* z, const float* mean, const float* invstd, const float* gamma,
                            const float* beta, const float* dbeta, const float* dgamma, float* dz, int64_t R, int C,
                            void* stream);
/* Replaces the backward of nn.MaxPool2d(3,2,1) and of adaptive_avg_pool2d + cat (models.py:224-245). */
int ssad_maxpool3x3s2_bwd(const float* x, const float* dy, float* dx, int64_t N, int H, int W, int C, int64_t dy_elems, void* stream);
/* Same pair with the argmax recorded by the forward pass (one byte per output element: window slot dy*3+dx of the
 * first maximum), so backward compares <= 4 indices per input element instead of rescanning 4 windows. */
int ssad_maxpool3x3s2_fwd_idx(const float* in, float* out, uint8_t* idx, int64_t N, int H, int W, int C, void* stream);
/* Stem tail / head of a TRAINING step, fused around the max-pool (models.py:224 under trainer.fit: bn1, relu, maxpool and
 * their autograd nodes).  Forward: BatchNorm (batch statistics mean / invstd already taken) + ReLU + max-pool 3x3/2 over
 * the raw conv1 output z [N][H][W][C]; only the pooled map and the argmax slots are written.  Backward: from the pooled
 * gradient dpool [N][Ho][Wo][C], the slots and z: dbeta, dgamma and dz (gradient of z) -- the max-pool backward, the
 * ReLU mask (recomputed from z) and both BatchNorm passes; the 128x128 activation and its gradient never exist in HBM.
 * workspace: ssad_colreduce_workspace(N*H*W, C) doubles. */
int ssad_bn_relu_maxpool_fwd(const float* z, const float* mean, const float* invstd, const float* gamma, const float* beta,
                             float* out, uint8_t* idx, int64_t N, int H, int W, int C, void* stream);
/* Round 5: the stem's BatchNorm backward reduction over the POOLED tensors.  ..._fwd_win also writes zwin[N][Ho][Wo][C], the raw z of each
 * window's winner; sum over pixels of g and g * xhat = sum over windows of dpool * mask(zwin) and dpool * mask * xhat(zwin) (a window
 * routes its gradient to exactly one pixel), i.e. ssad_bn_bwd_reduce_zmask(dpool, zwin, ...) over N * Ho * Wo rows; ..._bwd_apply is the
 * apply pass alone with dbeta / dgamma as inputs.  Half forms: ssad_bn_relu_maxpool_fwd_win_h, ssad_pool_bn_relu_bwd_apply_h. */
int ssad_bn_relu_maxpool_fwd_win(const float* z, const float* mean, const float* invstd, const float* gamma, const float* beta, float* out,
                                 uint8_t* idx, float* zwin, int64_t N, int H, int W, int C, void* stream);
int ssad_bn_relu_maxpool_fwd_win_h(const void* z, const float* mean, const float* invstd, const float* gamma, const float* beta, void* out,
                                   uint8_t* idx, void* zwin, int64_t N, int H, int W, int C, void* stream);
int ssad_pool_bn_relu_bwd_apply(const uint8_t* idx, const float* dpool, const float* z, const float* mean, const float* invstd,
                                const float* gamma, const float* beta, const float* dbeta, const float* dgamma, float* dz, int64_t N, int H,
                                int W, int C, int64_t dpool_elems, void* stream);
int ssad_pool_bn_relu_bwd_apply_h(const uint8_t* idx, const void* dpool, const void* z, const float* mean, const float* invstd,
                                  const float* gamma, const float* beta, const float* dbeta, const float* dgamma, void* dz, int64_t N, int H,
                                  int W, int C, int64_t dpool_elems, void* stream);
int ssad_pool_bn_relu_bwd(const uint8_t* idx, const float* dpool, const float* z, const float* mean, const float* invstd,
                          const float* gamma, const float* beta, float* dbeta, float* dgamma, float* dz, int64_t N, int H,
                          int W, int C, int64_t dpool_elems, double* workspace, void* stream);
int ssad_maxpool3x3s2_bwd_idx(const uint8_t* idx, const float* dy, float* dx, int64_t N, int H, int W, int C, int64_t dy_elems,
                              void* stream);
int ssad_gap_bwd(const float* dpooled, float* dy, int64_t N, int HW, int C, int stride, int offset, int accumulate,
                 void* stream);
/* Replaces F.cross_entropy + torchmetrics accuracy (models.py:261-262) and their backward: loss_acc[0] = mean NLL,
 * loss_acc[1] = accuracy, dlogits[b][0..ldd) = (softmax - onehot) * grad_scale (zero padded to ldd columns). */
int ssad_softmax_ce(const float* logits, const int64_t* labels, int B, int C, float* loss_acc, float* dlogits, int ldd,
                    float grad_scale, void* stream);
/* Replaces torch.optim.SGD(lr, momentum=0.9, weight_decay=5e-4).step() (models.py:337) over a flat parameter arena:
 * m = momentum*m + (g*grad_scale + weight_decay*p); p -= lr*m. */
int ssad_sgd_step(float* p, const float* g, float* m, int64_t n, float lr, float momentum, float weight_decay,
                  float grad_scale, void* stream);
/* The same update with its hyper-parameters in device memory -- hyper = [lr, momentum, weight_decay, grad_scale] -- so a
 * captured step (hipGraph) never bakes a learning rate in; `scaler` = NULL or the loss-scaler state below. */
int ssad_sgd_step_dev(float* p, const float* g, float* m, int64_t n, const float* hyper, const float* scaler, void* stream);
/* Dynamic loss scaling for the fp16-operand path: what torch.cuda.amp.GradScaler does for the reference under
 * pl.Trainer(precision=16) (tools.py:263).  scaler = 3 device floats [loss_scale, growth_tracker, found_inf]:
 * ssad_scale_by_loss_scale multiplies the loss gradient by loss_scale, ssad_check_finite sets found_inf when a gradient is
 * inf / nan, ssad_sgd_step_dev unscales (and skips the update while found_inf is set), ssad_loss_scaler_update applies
 * backoff / growth and clears found_inf. */
int ssad_scale_by_loss_scale(float* x, int64_t n, const float* scaler, void* stream);
int ssad_check_finite(const float* g, int64_t n, float* scaler, void* stream);
int ssad_loss_scaler_update(float* scaler, float growth_factor, float backoff_factor, int growth_interval, void* stream);

/* ---- synthetic-defect augmentation (batched, GPU resident) ---- */
/* One record per sample, drawn on the host in the reference's order (datasets.py:209-394): the GPU does the pixels,
 * with Pillow's own integer / float32 rules (self_supervised/pil_exact.py) so that the result is byte-identical to the
 * reference's PIL path.  All fields are 32-bit; the Python side mirrors this layout with a numpy structured dtype
 * (augment.py) and checks ssad_aug_params_size(). */
#define SSAD_AUG_MAX_LINE_POINTS 32
typedef struct ssad_aug_params {
    int32_t label;                          /* 0 good, 1 polygon patch, 2 scars, 3 poly-line */
    int32_t crop_left, crop_top;            /* output window origin inside the (affine) source image */
    int32_t aff_on;                         /* 0: no RandomAffine; 1: Image.transform(AFFINE, NEAREST) with the coefficients below */
    int32_t aff_fix[6];                     /* Pillow affine_fixed 16.16 integers: sx = (a2 + y a1 + x a0) >> 16, sy = (a5 + y a4 + x a3) >> 16 */
    int32_t cut_index, cut_left, cut_top, cut_w, cut_h;   /* defect source: index into `cuts` (-1 = the sample's own image) + window */
    int32_t patch_src_left, patch_src_top, patch_w, patch_h, patch_dst_left, patch_dst_top, patch_flat;
    int32_t patch_rgb[3];
    float   patch_bright[2];                /* two successive ImageEnhance.Brightness factors ... */
    int32_t patch_nbright;                  /* ... applied when this is 2 (0: none) */
    int32_t poly_n;
    int32_t poly_xy[16];                    /* up to 8 integer vertices in patch coordinates (ImageDraw.polygon) */
    int32_t scar_src_left, scar_src_top, scar_w, scar_h, scar_flat;
    int32_t scar_rgb[3];
    float   scar_bright[2];
    int32_t scar_nbright;
    int32_t scar_rot;                       /* 0: rotate() took the copy path (angle % 360 == 0); 1: affine_fixed coefficients below */
    int32_t scar_fix[6];
    int32_t scar_rw, scar_rh, scar_n;       /* rotated (expanded) size, number of pasted copies (<= 5) */
    int32_t scar_dst[10];                   /* left, top per copy */
    int32_t line_n;                         /* poly-line points (<= SSAD_AUG_MAX_LINE_POINTS), already (int)-truncated */
    int32_t line_xy[2 * SSAD_AUG_MAX_LINE_POINTS];
    int32_t line_quad[8 * (SSAD_AUG_MAX_LINE_POINTS - 1)];   /* width > 1: ImagingDrawWideLine's four vertices per segment */
    int32_t line_quad_ok[SSAD_AUG_MAX_LINE_POINTS - 1];      /* 0: degenerate segment (a single point) */
    int32_t line_rgb[3];
    int32_t line_width;
    int32_t jit_n;                          /* enabled ColorJitter ops, in application order: */
    int32_t jit_order[3];                   /* 0 brightness, 1 contrast, 2 saturation */
    float   jit_factor[3];                  /* indexed by op */
} ssad_aug_params;

int ssad_aug_params_size(void);
/* Replaces the PIL pixel work of PretextTaskDataset.__getitem__ (src/self_supervised/datasets.py:209-394;
 * dataset_generator.py:42-101, :268-275) for a whole batch: imgs [B][H][W][3] uint8 (and cuts [NC][H][W][3]) ->
 * out [B][3][h][w] fp32 normalised with mean3/std3 (host pointers) and, in `work` (B*h*w*3 bytes), the uint8 HWC image
 * BEFORE ColorJitter.  gray_mean: B floats of scratch. */
int ssad_cutpaste_augment(const uint8_t* imgs, const uint8_t* cuts, const ssad_aug_params* params, uint8_t* work,
                          float* gray_mean, float* out, int B, int H, int W, int h, int w, const float* mean3_host,
                          const float* std3_host, void* stream);
/* AnomalyDetector.predict (models.py:363-370) in one kernel: out[n] = mean of the k (1..3) smallest clip(1 - cos(x_n, bank_r), 0, 2)
 * over the R rows of an L2-normalised bank; the N x R similarity matrix is never written.  Bit-identical to
 * ssad_l2_normalize_rows -> ssad_conv_igemm_fwd (1x1) -> ssad_cosine_knn_mean.  D % 32 == 0. */
int ssad_cosine_knn_fused(const float* x, const float* bank_normalized, float* out, int64_t N, int D, int R, int k, void* stream);
/* AnomalyDetector.predict against a large bank (models.py:363-370 of the reference, scored over the whole normal training set):
 * ssad_cosine_knn_fused split over the bank rows.  Grid (ceil(N / 128), S); split s scores the bank rows [s rp, (s + 1) rp),
 * rp = 128 ceil(ceil(R / 128) / S), and writes the three smallest distances of each query to part [S][N][3] (caller-owned; INFINITY
 * where a split has fewer than three rows); a second launch merges the S triples per query in split order.  No float atomics.
 * Bit-identical to ssad_cosine_knn_fused for every S.  D % 32 == 0, 1 <= S <= 65535. */
int ssad_cosine_knn_split(const float* x, const float* bank_normalized, float* part, float* out, int64_t N, int D, int R, int k, int S,
                          void* stream);
/* kneighbors of the cosine bank (sklearn NearestNeighbors.kneighbors, which the reference's AnomalyDetector wraps, models.py:352-370,
 * returns (distances, indices); the two entries above keep the distances only).  Adds WHICH bank rows are the nearest: for every query
 * the k (1..3) smallest (distance, bank row) pairs in lexicographic order, ascending -- dist [N][k] float32, idx [N][k] int32; equal
 * distances go to the smaller row.  Tile, K order and distance expression of ssad_cosine_knn_fused: the distances are the bits it
 * averages.  S bank splits: 1 = one launch (part unused, may be null); S > 1 = the bank split of ssad_cosine_knn_split, part [S][N][3]
 * 64-bit keys (caller-owned, 8-byte aligned) + a merge launch.  No atomics; dist and idx are the same bits for every S and on every
 * call.  D % 32 == 0, D <= 65536, k <= R, 1 <= S <= 65535. */
int ssad_cosine_knn_index(const float* x, const float* bank_normalized, void* part, float* dist, int* idx, int64_t N, int D, int R,
                          int k, int S, void* stream);
/* Image scores at patch level (csrc/image_score.hip; PatchCore eq. 6-7 on cosine distances; the reference's patch-level branch
 * returns maps only).
 * ssad_rows_smallest_index adds a partial row sort: the bp = min(b, R) smallest (value, column) pairs of each row of m [Q][R],
 *   ascending, lexicographic (numpy's stable argsort; -0 counts as +0; no NaNs) -> vals [Q][bp], cols [Q][bp].  cosine != 0: the value
 *   of a column is clip(1 - m[q][c], 0, 2) (m holds similarities).  wgs workgroups per row over contiguous column ranges + one merge
 *   workgroup per row; part [Q][wgs][b] 64-bit keys (caller-owned, 8-byte aligned).  The result does not depend on wgs.
 *   1 <= b <= 32, 1 <= wgs <= 4096 / b, Q <= 65535.
 * ssad_rows_argmax adds a row maximum with its position: val[q] = max_p s[q][p], flat[q] = q P + the smallest p that reaches it.
 * ssad_knn_reweight adds the weight: out[q] = (1 - exp(d(x_q, mstar[q])) / sum_{j < bp} exp(d(x_q, nbr[q][j]))) smax[q] with
 *   d(x, r) = clip(1 - <x / ||x||, bank_r>, 0, 2), xs [Q][D] not normalised, bank L2-normalised, mstar [Q] and nbr [Q][bp] bank rows
 *   (a row outside 0 .. R - 1 counts as distance 1).  1 <= bp <= 32.  Fixed-order sums: the same bits on every call. */
int ssad_rows_smallest_index(const float* m, int64_t Q, int R, int b, int cosine, int wgs, void* part, float* vals, int* cols,
                             void* stream);
int ssad_rows_argmax(const float* s, int64_t Q, int P, float* val, int64_t* flat, void* stream);
int ssad_knn_reweight(const float* xs, const float* bank_normalized, const int* mstar, const int* nbr, const float* smax, float* out,
                      int64_t Q, int D, int R, int bp, void* stream);
/* The Euclidean metric of the kNN detector (csrc/knn_l2.hip; PatchCore's and SPADE's metric -- the reference has the cosine distance
 * only).  d(q, b) = sqrt(max(|q|^2 + |b|^2 - 2 <q, b>, 0)) on the raw rows, formed in fp32: <q, b> by the MFMA chain of the cosine
 * kernels (same tile, same K order) on unnormalised operands, the squared norms in the one summation order of ssad_row_sqnorms
 * (the query norms are taken inside the kernels in that order), d2 = fmaxf((qn + bn) - 2 dot, 0).  Selection runs on d2; sqrtf is
 * applied to the k winners only, so exact and near duplicates give finite distances >= 0.
 * ssad_row_sqnorms: out[n] = sum_j x[n][j]^2, one wave per row in one fixed order that does not depend on N or on where the row
 *   stands: equal rows give equal bits.  No atomics.
 * ssad_l2_knn_fused / _index: the cosine mean and index searches above with that distance -- out[n] = the mean of the k (1..3)
 *   smallest d, added smallest first; dist [N][k] / idx [N][k] = the k smallest (d2, bank row) pairs, lexicographic (equal d2 to the
 *   smaller row), dist = sqrtf(d2).  bank [R][D] not normalised, bank_sq [R] = ssad_row_sqnorms(bank).  S bank splits: 1 = one launch
 *   (part unused, may be null); S > 1 = part [S][N][3] floats (fused) or 64-bit keys (index, 8-byte aligned), caller-owned, and a merge
 *   launch.  out, dist and idx are the same bits for every S and on every call, and the k distances of the index form average to
 *   out's bits.  D % 32 == 0, D <= 65536, k <= R, 1 <= S <= 65535.
 * ssad_l2_from_dots: out[q][r] = max(qsq[q] + bsq[r] - 2 sim[q][r], 0), SQUARED distances from dot products sim [Q][R] (the
 *   expression above; feeds ssad_rows_smallest_index with cosine = 0).  out may be sim.  Q <= 65535.
 * ssad_knn_reweight_l2: ssad_knn_reweight for this metric: d(x, r) = sqrt(sum_j (x[j] - bank[r][j])^2) by direct differences, the
 *   weight in the shifted form 1 - exp(d(x_q, mstar[q]) - dmax) / sum_{j < bp} exp(d(x_q, nbr[q][j]) - dmax), dmax the largest of the
 *   bp neighbour distances (Euclidean distances are not bounded by 2; expf overflows above 88).  A row outside 0 .. R - 1 counts as
 *   distance 0.  1 <= bp <= 32. */
int ssad_row_sqnorms(const float* x, float* out, int64_t N, int D, void* stream);
int ssad_l2_knn_fused(const float* x, const float* bank, const float* bank_sq, float* part, float* out, int64_t N, int D, int R, int k,
                      int S, void* stream);
int ssad_l2_knn_index(const float* x, const float* bank, const float* bank_sq, void* part, float* dist, int* idx, int64_t N, int D,
                      int R, int k, int S, void* stream);
int ssad_l2_from_dots(const float* sim, const float* qsq, const float* bsq, float* out, int64_t Q, int R, void* stream);
int ssad_knn_reweight_l2(const float* xs, const float* bank, const int* mstar, const int* nbr, const float* smax, float* out, int64_t Q,
                         int D, int R, int bp, void* stream);
/* Half-precision operands for the flat Euclidean search (csrc/knn_l2_half.hip; faiss' GpuIndexFlat useFloat16): the distance of the
 * rows ROUNDED to fp16, d = sqrt(max(|h(q)|^2 + |h(b)|^2 - 2 <h(q), h(b)>, 0)), the dot product on v_mfma_f32_32x32x16_f16 (fp16
 * products, fp32 accumulation).  h: fp32 -> fp16, round to nearest even, saturating at +-65504, results of magnitude below 2^-14
 * flushed to signed zero: no half holds inf, NaN or a subnormal.
 * ssad_rows_to_half: xh[n][j] = h(x[n][j]) (xh: [N][D] halves) and sq[n] = sum_j xh[n][j]^2 in fp32 in ssad_row_sqnorms' order, one
 *   pass: equal rounded rows give equal norm bits wherever they stand.  D % 32 == 0, D <= 65536.
 * ssad_l2h_knn_fused / _index: ssad_l2_knn_fused / _index on rounded rows -- xh [N][D] and bankh [R][D] halves (16-byte aligned),
 *   x_sq [N] and bank_sq [R] their norms from ssad_rows_to_half; out, dist, idx, part, S, k and the bit claims (the same bits for
 *   every S and on every call; the index form's distances average to out's bits) as there. */
int ssad_rows_to_half(const float* x, void* xh, float* sq, int64_t N, int D, void* stream);
int ssad_l2h_knn_fused(const void* xh, const float* x_sq, const void* bankh, const float* bank_sq, float* part, float* out, int64_t N,
                       int D, int R, int k, int S, void* stream);
int ssad_l2h_knn_index(const void* xh, const float* x_sq, const void* bankh, const float* bank_sq, void* part, float* dist, int* idx,
                       int64_t N, int D, int R, int k, int S, void* stream);
/* An 8-bit scalar-quantised bank for the flat Euclidean search (csrc/knn_l2_int8.hip; faiss' IndexScalarQuantizer, QT_8bit_uniform):
 * one affine code (lo, s) for the whole bank, c(x) = rint(min(max((x - lo) * inv_s, 0), 255)) - 128 in fp32 in that order (to nearest
 * even; NaN -> -128), stored as int8.  The distance is that BETWEEN THE CODES plus the query's clamp loss:
 * d = sqrtf(fmaf(s2, (float)D2, excess)), D2 = sum_j (c(q_j) - c(b_j))^2 = (qsq + bsq) - 2 <c(q), c(b)> in int32 -- exact, the dot
 * product on v_mfma_i32_32x32x32_i8 -- and s2 = s s rounded once by the caller.
 * ssad_rows_to_int8: codes [N][D] int8 (8-byte aligned; x 16-byte aligned), sq[n] = sum_j codes[n][j]^2 (int32) and excess[n] =
 *   sum_j (x[n][j] - min(max(x[n][j], lo), fmaf(255, s, lo)))^2 in fp32 in ssad_row_sqnorms' order (0 for a row inside the coded
 *   range, NaN for a row with a NaN), one pass.  D % 32 == 0, D <= 32768 (D 255^2 must fit int32).
 * ssad_l2q_knn_fused / _index: ssad_l2_knn_fused / _index on codes, k = 1..3 -- xq [N][D] and bankq [R][D] codes (16-byte aligned),
 *   x_sq [N], x_excess [N] and bank_sq [R] from ssad_rows_to_int8.  S bank splits: 1 = one launch (part unused); S > 1 = part
 *   [S][N][3] uint32 (fused) or 64-bit keys (index), caller-owned, 8-byte aligned, and a merge launch.  idx: equal D2 to the smaller
 *   row -- the first k entries of a stable sort of (D2, row), exactly.  The same bits for every S and on every call; out is the
 *   sequential fp32 sum of the index form's dist row divided by k.  Every error leaves the outputs untouched. */
int ssad_rows_to_int8(const float* x, void* codes, int* sq, float* excess, int64_t N, int D, float lo, float inv_s, float s,
                      void* stream);
int ssad_l2q_knn_fused(const void* xq, const int* x_sq, const float* x_excess, const void* bankq, const int* bank_sq, void* part,
                       float* out, int64_t N, int D, int R, int k, int S, float s2, void* stream);
int ssad_l2q_knn_index(const void* xq, const int* x_sq, const float* x_excess, const void* bankq, const int* bank_sq, void* part,
                       float* dist, int* idx, int64_t N, int D, int R, int k, int S, float s2, void* stream);
/* The flat Euclidean search for k = 4..32 (csrc/knn_topk.hip; the entry points above keep k = 1..3): the same tile, dot loops, norms
 * and d2 expression, so a (query, bank row) pair has the d2 bits of ssad_l2_knn_index / ssad_l2h_knn_index; a query keeps the k
 * smallest (d2 bits << 32 | row) keys.  Keys are unique: the result is the first k entries of a stable ascending sort of (d2, row)
 * whatever the split count S and the batch a query sits in, the same bits on every call.  No atomics.
 * ssad_l2_knn_topk_index: dist [N][k] = sqrtf(d2) of the winners, idx [N][k] int32, ascending, equal d2 to the smaller row.
 * ssad_l2_knn_topk: out[n] = (dist[n][0] + dist[n][1] + ... + dist[n][k - 1]) / k, added in that order in fp32.
 * ssad_l2h_knn_topk / _index: the same on rounded rows (arguments as ssad_l2h_knn_fused).
 * S bank splits, 1 <= S <= 65535 (1: one launch; else a merge launch follows); part [S][N][k] 64-bit keys, caller-owned, 8-byte
 * aligned, unused (may be null) for S = 1.  D % 32 == 0, D <= 65536, 4 <= k <= 32, k <= R. */
int ssad_l2_knn_topk(const float* x, const float* bank, const float* bank_sq, void* part, float* out, int64_t N, int D, int R, int k,
                     int S, void* stream);
int ssad_l2_knn_topk_index(const float* x, const float* bank, const float* bank_sq, void* part, float* dist, int* idx, int64_t N, int D,
                           int R, int k, int S, void* stream);
int ssad_l2h_knn_topk(const void* xh, const float* x_sq, const void* bankh, const float* bank_sq, void* part, float* out, int64_t N,
                      int D, int R, int k, int S, void* stream);
int ssad_l2h_knn_topk_index(const void* xh, const float* x_sq, const void* bankh, const float* bank_sq, void* part, float* dist,
                            int* idx, int64_t N, int D, int R, int k, int S, void* stream);
/* Refining a coarse shortlist with exact fp32 distances (csrc/knn_refine.hip; faiss' IndexRefineFlat): x [N][D] fp32 queries, bank
 * [R][D] fp32 rows, cand [N][r] int32 listed bank rows of every query (1 <= r <= 32), any D >= 1.
 * ssad_rerank_l2_index: for query n the first k (1 <= k <= r) entries of an ascending sort of its listed rows by (d2 bits, bank row,
 *   place in the list), d2 = sum_c (x_c - b_c)^2 with ssad_l2_direct's bits (lane l of a wave: elements l, l + 64, ... in an fma
 *   chain, then the xor butterfly) -- they do not depend on N, r, the place in the list or the batch.  dist [N][k] = sqrtf(d2), idx
 *   [N][k] the bank row.  An entry outside 0 .. R - 1 is skipped; a query with fewer than k valid entries gets (+inf, -1) in the
 *   missing places; a row listed twice APPEARS TWICE (nothing is deduplicated).
 * ssad_rerank_l2: out[n] = (dist[n][0] + ... + dist[n][k - 1]) / k, added in that order in fp32 (+inf with fewer than k valid entries).
 * No atomics, selection by rank counting: the same bits on every call.  Every error returns before a launch, outputs untouched.
 * ssad_topk_l2q_index: ssad_l2q_knn_index for k = 4..32 (arguments as there; part [S][N][k] 64-bit keys, caller-owned, 8-byte
 *   aligned, unused for S = 1): idx is exactly the first k entries of a stable ascending sort of (D2, row), D2 the integer squared
 *   code distance, dist = sqrtf(fmaf(s2, (float)D2, excess)); the first three columns are ssad_l2q_knn_index(k = 3) bit for bit, the
 *   same bits for every S.  D % 32 == 0, D <= 32768, 4 <= k <= 32, k <= R, codes 16-byte aligned. */
int ssad_rerank_l2_index(const float* x, const float* bank, const int* cand, float* dist, int* idx, int64_t N, int D, int R, int r,
                         int k, void* stream);
int ssad_rerank_l2(const float* x, const float* bank, const int* cand, float* out, int64_t N, int D, int R, int r, int k, void* stream);
int ssad_topk_l2q_index(const void* xq, const int* x_sq, const float* x_excess, const void* bankq, const int* bank_sq, void* part,
                            float* dist, int* idx, int64_t N, int D, int R, int k, int S, float s2, void* stream);
/* SPADE's image-conditioned gallery for the Euclidean kNN (csrc/knn_gallery.hip; Cohen & Hoshen 2020): a query image is scored against
 * the rows of K bank images only.  Queries x [Q P][D] and bank [T P][D] hold P rows per image, image after image.
 * ssad_group_means: out[g][c] = mean_i x[g P + i][c], the image descriptor: summed in fp64 in row order 0 .. P - 1, rounded once to
 *   fp32 -- an image's descriptor is the same bits in every batch.  G <= 65535.
 * ssad_l2_direct: out[q][t] = sum_c (q[q][c] - b[t][c])^2 by direct differences (no cancellation), one wave per pair in the order
 *   of ssad_row_sqnorms (lane-strided fma chain, xor butterfly): a pair's bits do not depend on Q or T.  Q <= 65535.
 * ssad_l2_knn_gallery / _index: ssad_l2_knn_fused / ssad_l2_knn_index with the bank of query image q restricted to the row blocks
 *   [g P, (g + 1) P), g = gallery[q][0 .. K - 1] (int32 bank-image ids).  Grid (ceil(P / 128), Q, S): a query tile never straddles two
 *   images, a bank tile never two blocks.  A (query, bank row) pair gets the bits the whole-bank kernels give it: the same tile functions
 *   (csrc/knn_tile.h) -- K order, norms and d2 = fmaxf((qn + bn) - 2 dot, 0).  idx holds GLOBAL bank rows, equal d2 go to the smaller global row.  An entry outside
 *   0 .. T - 1 is skipped, never dereferenced; a query left with fewer than k candidates gets out = +inf, the missing slots of the
 *   index form (+inf, -1).  S >= 1 splits the K entries; S > 1 needs part ([S][Q P][3] floats / 64-bit keys, 8-byte aligned) and a
 *   merge launch.  out, dist and idx are the same bits for every S and on every call.  D % 32 == 0, D <= 65536, k in 1..3,
 *   K P >= k, Q <= 65535, T P < 2^31. */
int ssad_group_means(const float* x, float* out, int64_t G, int P, int D, void* stream);
int ssad_l2_direct(const float* q, const float* b, float* out, int64_t Q, int T, int D, void* stream);
int ssad_l2_knn_gallery(const float* x, const float* bank, const float* bank_sq, const int* gallery, float* part, float* out, int Q,
                        int P, int T, int K, int D, int k, int S, void* stream);
int ssad_l2_knn_gallery_index(const float* x, const float* bank, const float* bank_sq, const int* gallery, void* part, float* dist,
                              int* idx, int Q, int P, int T, int K, int D, int k, int S, void* stream);
/* An inverted-file (IVF-Flat) index for the Euclidean kNN (csrc/knn_ivf.hip; PatchCore's approximate search, faiss' IndexIVFFlat):
 * the bank rows are clustered into nlist cells and stored cell after cell (bank [R][D] sorted by cell, offsets [nlist + 1], perm [R]
 * the original row of every sorted row); a query meets the rows of the cells probes[n][0 .. nprobe - 1] only.
 * ssad_segment_means: out[g][c] = mean of x[order[i]][c], i = offsets[g] .. offsets[g + 1] - 1 (k-means' update step; order int32
 *   [N], the rows sorted by cell): summed in fp64 in order's sequence, rounded once to fp32, no atomics -- the same bits on every
 *   call.  An empty segment leaves out[g] untouched.  nlist <= 65535.
 * ssad_l2_knn_ivf / _index: ssad_l2_knn_fused / ssad_l2_knn_index over the probed cells.  The work list is made by the caller on
 *   the device: pairs [N nprobe] = the pair ids n nprobe + j sorted by the cell they name, tiles [3][G] = cell, first pair and number
 *   of pairs (1 .. 128) of every tile, a tile never straddling two cells; G is an upper bound (N nprobe / 128 + nlist), a tile whose
 *   cell is outside 0 .. nlist - 1 exits at once.  Launch 1, grid (G): one cell x up to 128 gathered queries per workgroup, the
 *   128 x 128 tile of ssad_l2_knn_index; part [N nprobe][3] 64-bit keys (squared-distance bits << 32 | original row), 8-byte aligned.
 *   Launch 2 merges the nprobe triples of every query.  A (query, bank row) pair gets the bits the whole-bank kernels give it,
 *   whichever tile it falls into; idx holds ORIGINAL rows (perm), equal d2 go to the smaller original row; a probe entry outside
 *   0 .. nlist - 1 is skipped; slots the probed cells cannot fill hold (+inf, -1), out = +inf.  Every index read from device memory
 *   is checked before it addresses anything.  D % 32 == 0, D <= 65536, k in 1..3, N nprobe < 2^31, x 16-byte aligned. */
int ssad_segment_means(const float* x, const int* order, const int* offsets, float* out, int64_t N, int nlist, int D, void* stream);
int ssad_l2_knn_ivf(const float* x, const float* bank, const float* bank_sq, const int* offsets, const int* perm, const int* probes,
                    const int* tiles, const int* pairs, void* part, float* out, int64_t N, int D, int R, int nlist, int nprobe, int G,
                    int k, void* stream);
int ssad_l2_knn_ivf_index(const float* x, const float* bank, const float* bank_sq, const int* offsets, const int* perm, const int* probes,
                          const int* tiles, const int* pairs, void* part, float* dist, int* idx, int64_t N, int D, int R, int nlist,
                          int nprobe, int G, int k, void* stream);
/* Locally aware patch features from two stage maps of one trunk pass (csrc/patch_features.hip).  Replaces nothing in the reference,
 * which scores 841 windows per image (models.py:211-219); this is the feature construction of PatchCore (Roth et al., CVPR 2022,
 * section 3.1) as anomalib implements it: AvgPool2d(3, 1, 1) of every stage map, F.interpolate(mode='bilinear', align_corners=False)
 * of the coarser one to the finer grid, channels concatenated.
 *   fine [N][Hf][Wf][Cf], coarse [N][Hc][Wc][Cc] NHWC fp32 -> out [N * Hf * Wf][Cf + Cc], rows in (n, i, j) order, not normalised:
 *   columns [0, Cf): 1/9 of the 3 x 3 neighbourhood sum of fine (zeros outside the map); columns [Cf, Cf + Cc): the bilinear blend of
 *   the pooled coarse map P at y0, y1, x0, x1 with num = max((2 i + 1) Hc - Hf, 0), y0 = num div (2 Hf), y1 = min(y0 + 1, Hc - 1),
 *   ly = (num - y0 2 Hf) / (2 Hf) (columns likewise): integer sample positions, correctly rounded weights.
 *   Cf % 4 == 0, Cc % 4 == 0, 16-byte aligned pointers, map sides in 1 .. 32768, Wc <= 2048, any ratio of the two sizes.
 *   rows_per_block: fine rows of one image a workgroup walks down, 0 = chosen by the library; the result does not depend on it.
 *   No atomics, fixed summation order: the same bits on every call. */
int ssad_local_patch_features(const float* fine, const float* coarse, float* out, int64_t N, int Hf, int Wf, int Cf, int Hc, int Wc,
                              int Cc, int rows_per_block, void* stream);
/* Stage-pyramid rows from two or three stage maps of one trunk pass (csrc/pyramid_features.hip).  Replaces nothing in the reference;
 * this is the embedding of PaDiM (Defard et al., ICPR 2020; anomalib's PadimModel) and of SPADE's pixel stage: the stage maps as they
 * are, the coarser ones replicated (nearest neighbour) to the finest grid, channels concatenated, optionally only chosen columns kept.
 *   m0, m1, m2 [N][H_s][W_s][C_s] NHWC fp32, finest first (stages = 2: m2 is not read); D = C0 + C1 (+ C2);
 *   sel [d] int32 on the device, strictly increasing entries in [0, D) (the caller checks them), or NULL = all D columns (d == D)
 *   -> out [N * H0 * W0][d], rows in (n, i, j) order:
 *   out[(n, i, j)][k] = m_s[n][(i H_s) div H0][(j W_s) div W0][c], s the stage of column sel[k], c its channel there.
 *   A pure copy with integer source indices (F.interpolate(mode='nearest') where the ratios are integers); a column nobody chose is
 *   never written.  C_s % 4 == 0, H0 >= H1 >= H2, W0 >= W1 >= W2, any ratio, map sides in 1 .. 32768, stages * W0 + d <= 16384; the
 *   maps 16-byte aligned, out as well when d % 4 == 0.
 *   rows_per_block: fine rows of one image a workgroup walks down, 0 = chosen by the library; the result does not depend on it.
 *   No atomics: the same bits on every call, for every N. */
int ssad_stage_pyramid_rows(const float* m0, const float* m1, const float* m2, const int* sel, float* out, int64_t N, int stages,
                            int H0, int W0, int C0, int H1, int W1, int C1, int H2, int W2, int C2, int d, int rows_per_block,
                            void* stream);
/* Greedy k-center (farthest-point) coreset of the kNN bank (PatchCore; csrc/coreset.hip; the reference has no coreset) over the
 * rows of p [R][d] (fp32, row-major), squared Euclidean distance sum_j (p[r][j] - p[c][j])^2 summed as a direct sum of squared
 * differences in one fixed order per row.  sel[0] = start; sel[t] = argmax_r min_{s<t} dist(r, sel[s]), ties to the smallest row;
 * rad[t] = that maximum (rad[0] = +inf).  Stops early when the maximum reaches 0 (every row lies on a centre): *m_out (written on
 * the device, read by the caller after the stream) is the number of centres recorded, <= min(m, R).  One launch per step on
 * `wgs` workgroups of contiguous rows, the last step on one; no atomics.  sel, rad and *m_out are the same bits for every wgs.
 * Workspace (caller-owned): mind [R] floats, part [2][wgs] (float value, int32 row) pairs.  sel / rad hold min(m, R) entries.
 * d % 4 == 0, 4 <= d <= 1024, p 16-byte aligned, finite rows. */
int ssad_coreset_greedy(const float* p, int64_t R, int d, int m, int64_t start, int wgs, float* mind, void* part, int64_t* sel,
                        float* rad, int* m_out, void* stream);
/* Gaussian density estimator (GDE) scorer of CutPaste (csrc/gde.hip; the reference has no such scorer).
 * ssad_gaussian_fit_stats: of the N rows of x [N][D] (each first L2-normalised bit-identically to ssad_l2_normalize_rows when
 * `normalize`), in fp64: mean[D], scatter[D][D] = sum_i (x_i - mean)(x_i - mean)^T and m4[0] = sum_i ||x_i - mean||^4 (the sufficient
 * statistics of sklearn's Ledoit-Wolf shrinkage).  Fixed-order reductions: the same bits on every call.  N >= 1, D % 32 == 0,
 * 32 <= D <= 4096.
 * ssad_mahalanobis_fused: out[i] = ||W (x_i - mu)||_2 in one kernel on the fp32 matrix cores, mu = mu_hi + mu_lo (a float pair:
 * (x - mu_hi) - mu_lo), W [D][D] the lower-triangular inverse Cholesky factor of the shrunk covariance (its upper triangle is not
 * read: it may hold anything, NaN included); x_i optionally L2-normalised as above.  No split across workgroups: a row's score does
 * not depend on N or on its position.  D % 32 == 0, 32 <= D <= 1024. */
int ssad_gaussian_fit_stats(const float* x, int64_t N, int D, int normalize, double* mean, double* scatter, double* m4, void* stream);
int ssad_mahalanobis_fused(const float* x, const float* mu_hi, const float* mu_lo, const float* w, float* out, int64_t N, int D,
                           int normalize, void* stream);
/* Per-position Gaussian detector (PaDiM, Defard et al. ICPR 2020; csrc/padim.hip; the reference has no such scorer) on dense rows
 * x [n_img * P][D], row n P + p = position p of image n; sel [d] int32 on the device picks d of the D columns (every entry in
 * [0, D): the caller checks it).
 * ssad_position_gaussian_fit_stats: per position, in fp64, mean[P][d] and scatter[P][d][d] = sum_n c c^T of the centred selected
 *   columns; images summed in ascending order, each 64 x 64 tile of the lower triangle mirrored exactly, no atomics: the same bits on
 *   every call.  n_img >= 2.
 * ssad_position_mahalanobis: out[n P + p] = ||W_p (x_sel - mu_p)||_2 in one kernel on the fp32 matrix cores, mu_p = mu_hi[p] +
 *   mu_lo[p] ([P][d] float pairs: (x - mu_hi) - mu_lo), W_p = w[p] [d][d] lower triangular (whatever its upper triangle holds is never
 *   used).  A workgroup owns one position and 128 images and runs over all of W_p: a score does not depend on n_img or on where its
 *   image sits in the launch.  d <= 1024, 512 (P + 1) D <= 2^31, sel / mu_hi / mu_lo / w 16-byte aligned.
 * Both: d % 32 == 0, 32 <= d <= D, D % 4 == 0, P >= 1, n_img >= 1; anything else returns the argument error without a launch. */
int ssad_position_gaussian_fit_stats(const float* x, const int* sel, int n_img, int64_t P, int D, int d, double* mean, double* scatter,
                                     void* stream);
int ssad_position_mahalanobis(const float* x, const int* sel, const float* mu_hi, const float* mu_lo, const float* w, float* out,
                              int n_img, int64_t P, int D, int d, void* stream);
/* The step between the two above, on the device (csrc/padim.hip): per position p, all in fp64,
 *   Sigma = scatter[p] / (n - 1) + eps I,  C = the lower Cholesky factor of Sigma,  W = C^-1 (lower triangular).
 * mean [P][d] and scatter [P][d][d] are what ssad_position_gaussian_fit_stats wrote.  Only the lower triangle of scatter (diagonal
 * included) is read; scatter is the WORKSPACE and is overwritten, Sigma -> C -> W in place in that triangle (LAPACK's potrf +
 * trtri), the upper triangle is neither read nor written.
 * Out: w [P][d][d] fp32 = W rounded once, exact +0.0f above the diagonal; mu_hi = fp32(mean), mu_lo = fp32(mean - mu_hi) (the float
 * pair ssad_position_mahalanobis takes); c_out / w64_out [P][d][d] fp64 (either may be NULL) = C / W before the rounding, zeros above
 * the diagonal; info [P] = 0, or 1 + the column of the first pivot that is not finite and positive (LAPACK's info).  A position with
 * info != 0 has w (and c_out, w64_out) filled with NaN and its mu written; the other positions are not affected.  A bad pivot is a
 * status: the kernel neither loops nor traps on it.
 * Arithmetic: fp64 FMA only, nothing in fp32 before the final rounding.  Every element is (a - sum_k l_k b_k) / pivot as one fma
 * chain with k ascending and a true division; one workgroup owns one matrix, no atomics and no sum split across workgroups: the same
 * bits on every call, and position p of a P-position launch equals the same matrix launched as P = 1.
 * d % 32 == 0, 32 <= d <= 512; 1 <= P < 2^31; n >= 2; eps > 0; no pointer NULL but c_out / w64_out; anything else returns the
 * argument error without a launch. */
int ssad_position_gaussian_factor(const double* mean, double* scatter, int64_t P, int d, int64_t n, double eps, float* mu_hi,
                                  float* mu_lo, float* w, double* c_out, double* w64_out, int* info, void* stream);
/* HOST function (no GPU work): per-channel integer sums of the window [top, top + h) x [left, left + w) of the NEAREST affine
 * transform of an H x W x 3 uint8 image (fix: the six 16.16 coefficients of ssad_aug_params.aff_fix; NULL: the image itself),
 * zero outside the image.  The sampler's colour-similarity test (datasets.py:300-312) needs this mean between two random
 * draws. */
int ssad_affine_window_sum_u8(const uint8_t* img, int H, int W, const int32_t* fix, int left, int top, int w, int h,
                              int64_t* sum3);
/* The other sort-bound metrics of an evaluation, for maps that are already on the device (same hand-written radix sort as
 * ssad_auroc; no library sort).
 * ssad_pro_curve: the MVTec per-region-overlap curve of metrics.compute_pro (src/self_supervised/metrics.py:58-190): scores fp32
 *   [n]; fp_w uint8 [n] = 1 on defect-free pixels; pro_w fp64 [n] = 1 / (size of the pixel's ground-truth region), 0 elsewhere;
 *   n_ok = number of defect-free pixels, n_regions = number of regions (each at least 1, numpy's max(., 1)).  Writes one curve
 *   point per distinct score in descending order -- fprs fp32, pros fp64, both clipped at 1 -- and their number to count[0]
 *   (device memory; the arrays need room for n entries).  The caller adds the end points (0, 0) and (1, 1).
 * ssad_best_f1_threshold: the threshold maximising F1 over torchmetrics' precision-recall curve (tools.py:141-146), float32
 *   arithmetic as there, the smallest threshold among equal F1.  targets: 1 = positive.  out[0] = threshold, out[1] = F1.
 * ssad_confusion_counts: tp, fp, fn, tn of (scores >= threshold) against (targets != 0), added into out[0..3] (int64, zeroed by
 *   the caller): what compute_f1 / compute_iou (tools.py:131-139) need. */
int64_t ssad_pro_curve_workspace(int64_t n);
int ssad_pro_curve(const float* scores, const uint8_t* fp_w, const double* pro_w, int64_t n, double n_ok, double n_regions,
                   void* workspace, int64_t workspace_bytes, float* fprs, double* pros, int64_t* count, void* stream);
int64_t ssad_best_f1_workspace(int64_t n);
int ssad_best_f1_threshold(const float* scores, const uint8_t* targets, int64_t n, void* workspace, int64_t workspace_bytes, float* out,
                           void* stream);
int ssad_confusion_counts(const float* scores, const uint8_t* targets, int64_t n, float threshold, int64_t* out, void* stream);
/* Average precision and the precision-recall curve of device-resident scores.  The reference has no AP (its Evaluator stops at
 * AUROC / F1 / AUPRO / IoU); this replaces what a user would otherwise call on the host, sklearn.metrics.average_precision_score /
 * precision_recall_curve.  Same radix sort as ssad_auroc, descending, the target as payload; scores fp32 [n], targets uint8 [n],
 * non-zero = positive.  A threshold is a distinct score value (-0.0 and +0.0 are one value; NaN scores are not defined).  For the
 * j-th distinct value in descending order, TP_j = positives with a score >= it, N_j = elements with a score >= it, P = TP_m:
 *   AP = sum_j (TP_j - TP_{j-1}) / P * TP_j / N_j   (TP_0 = 0; sklearn's step-wise sum, no trapezoid; P = 0 gives AP = 0.0, the
 *   value of sklearn's arithmetic with its "recall is set to one" convention).
 * ssad_average_precision: out[0] = AP, out[1] = P, out[2] = m, the number of distinct scores.  Exact integer counts; every term is
 *   formed in fp64 and the terms are summed per workgroup and then over the workgroups in an order fixed by n: no floating-point
 *   atomics, the same bits on every call and for every order of the input.
 * ssad_pr_curve: one point per distinct score in DESCENDING threshold order: precision = TP_j / N_j and recall = TP_j / P (1.0
 *   when P = 0) fp64, thresholds fp32 (a run of zeros reports -0.0 when it holds one); their number goes to count[0] (device
 *   memory; the arrays need room for n entries).  The caller appends sklearn's end point (precision 1, recall 0) and reverses.
 * The workspace holds ssad_*_workspace(n) bytes (-1 for n <= 0 or n >= 2^31 - 1) and is aligned to 8 bytes.  A null pointer, n <= 0,
 * a workspace too small or misaligned returns 2 with ssad_last_error() set, before anything is written. */
int64_t ssad_average_precision_workspace(int64_t n);
int ssad_average_precision(const float* scores, const uint8_t* targets, int64_t n, void* workspace, int64_t workspace_bytes,
                           double* out, void* stream);
int64_t ssad_pr_curve_workspace(int64_t n);
int ssad_pr_curve(const float* scores, const uint8_t* targets, int64_t n, void* workspace, int64_t workspace_bytes,
                  double* precision, double* recall, float* thresholds, int64_t* count, void* stream);

/* transforms.ToTensor() on a uint8 HWC batch: -> [B][3][H][W] fp32 in [0,1] (the Dataset's third output). */
int ssad_u8hwc_to_f32chw(const uint8_t* img, float* out, int B, int H, int W, void* stream);
/* The transform of MVTecDataset.__getitem__ (datasets.py:68-80, :102-105: ToTensor, then Normalize(mean, std)) on a uint8 HWC
 * batch that is already on the device: orig (may be NULL) = img / 255, norm = (img / 255 - mean) / std, both [B][3][H][W], each
 * operation a single IEEE fp32 operation as torch evaluates them on the host (bit-identical).  mean3 / std3: host pointers. */
int ssad_u8hwc_to_f32chw_norm(const uint8_t* img, float* orig, float* norm, int B, int H, int W, const float* mean3_host,
                              const float* std3_host, void* stream);

/* Image.resize(size) of Pillow (default filter: BICUBIC) for 8-bit 'L' (C = 1) / 'RGB' (C = 3) batches already on the device:
 * what the reference applies to every file it opens (datasets.py:68, :211-213, :189-200).  in [B][Hin][Win][C] -> out
 * [B][Hout][Wout][C]; tmp [B][Hin][Wout][C] when both extents change (else may be NULL).  bounds_* int32 [out][2] = (first source
 * index, taps) and coef_* int32 [out][ksize_*] (22-bit fixed point) are DEVICE arrays holding libImaging's precompute_coeffs +
 * normalize_coeffs_8bpc tables (self_supervised/pil_exact.resample_coeffs); the axis whose extent does not change takes no table.
 * Bit-exact integer arithmetic (Resample.c, ImagingResampleHorizontal_8bpc / Vertical_8bpc). */
int ssad_resize_bicubic_u8(const uint8_t* in, uint8_t* tmp, uint8_t* out, int B, int Hin, int Win, int C, int Hout, int Wout,
                           const int32_t* bounds_x, const int32_t* coef_x, int ksize_x, const int32_t* bounds_y,
                           const int32_t* coef_y, int ksize_y, void* stream);

/* dataset_generator.obj_mask (dataset_generator.py:27-39: skimage.feature.canny(sigma = 1.5, low 5, high 15) -> binary dilation 3 x 3
 * -> closing 3 x 3 -> fill holes -> erosion 4 x 4 -> largest 8-connected component) for a uint8 RGB batch on the device:
 * rgb [B][H][W][3] -> mask [B][H][W] (0 / 1) and edges [B][H][W] (the Canny edge map, 0 / 1).  gauss_w_host: the 2 * radius + 1
 * normalised Gaussian weights as scipy.ndimage computes them (host memory); low / high: the thresholds on the [0, 1] scale.
 * workspace: ssad_obj_mask_workspace(B, H, W) bytes of device memory.  Bit-exact against the host statement (fp64, scipy's
 * operation order, glibc's hypot restated; fixed points for hysteresis / filling / labelling). */
int64_t ssad_obj_mask_workspace(int B, int H, int W);
int ssad_obj_mask(const uint8_t* rgb, uint8_t* mask, uint8_t* edges, int B, int H, int W, const double* gauss_w_host, int radius,
                  double low, double high, void* workspace, void* stream);

/* Defect regions (csrc/regions.hip): what a user does with an anomaly map after the threshold.  All outputs are integers (and
 * min / max of the scores): exact, and the same bits on every call.
 * ssad_label_regions: connected components of a batch of binary images [n][H][W].  Foreground is EITHER scores fp32 with
 *   scores >= threshold (the rule of ssad_confusion_counts: NaN is background, +inf >= +inf is foreground) OR mask uint8 != 0;
 *   exactly one of the two pointers is non-NULL.  connectivity: 8 or 4.  labels int32 [n][H][W]: 0 = background, components
 *   numbered 1 .. counts[i] per image in raster order of their first pixel -- scipy.ndimage.label's array exactly; counts int32
 *   [n]; offsets int32 [n + 1] = exclusive prefix sum of counts.  n, H, W >= 1, H * W < 2^30, n * H * W < 2^31.  workspace:
 *   ssad_label_regions_workspace(n, H, W) bytes.  A union-find over pixel indices in tiles of ssad_label_regions_tile() pixels a
 *   side (LDS), merged across tile borders by atomic minima: the work does not grow with the length of a component's path.
 * ssad_region_stats: with R = offsets[n] (read back by the caller; R = 0 writes nothing), per region in (image, label) order:
 *   area int32 [R]; bbox int32 [R][4] = x0, y0, x1, y1 with inclusive maxima; coord_sum int64 [R][2] = sum of x, sum of y (the
 *   centroid as an exact rational); and, when scores is given (else all three NULL), peak fp32 [R] = the largest score of the
 *   region and peak_pos int32 [R] = the smallest raster index within the image that attains it (NaN orders below every number).
 * ssad_region_filter: mask_out uint8 [n][H][W] = 1 where the pixel's region r has keep[r] != 0 (keep uint8 [R]).  With labels_out
 *   (may be labels itself), counts_out [n] and offsets_out [n + 1] (all three or none): the kept regions renumbered 1 .. per
 *   image in the same order; then workspace holds ssad_region_filter_workspace(R) bytes.
 * ssad_pro_weights: the two planes of ssad_pro_curve from labelled ground truths: fp_w uint8 = (label == 0), pro_w fp64 = 1.0 /
 *   area of the pixel's region (the correctly rounded quotient), 0 on background.
 * A bad argument returns 2 before any launch. */
int ssad_label_regions_tile(void);
int64_t ssad_label_regions_workspace(int64_t n, int H, int W);
int ssad_label_regions(const float* scores, float threshold, const uint8_t* mask, int64_t n, int H, int W, int connectivity,
                       int32_t* labels, int32_t* counts, int32_t* offsets, void* workspace, int64_t workspace_bytes, void* stream);
int ssad_region_stats(const float* scores, const int32_t* labels, const int32_t* offsets, int64_t n, int H, int W, int64_t R,
                      int32_t* area, int32_t* bbox, int64_t* coord_sum, float* peak, int32_t* peak_pos, void* stream);
int64_t ssad_region_filter_workspace(int64_t R);
int ssad_region_filter(const int32_t* labels, const int32_t* offsets, const uint8_t* keep, int64_t n, int H, int W, int64_t R,
                       uint8_t* mask_out, int32_t* labels_out, int32_t* counts_out, int32_t* offsets_out, void* workspace,
                       int64_t workspace_bytes, void* stream);
int ssad_pro_weights(const int32_t* labels, const int32_t* offsets, const int32_t* area, int64_t n, int H, int W, uint8_t* fp_w,
                     double* pro_w, void* stream);

/* Anomaly maps as PatchCore and PaDiM define them (csrc/resize_gaussian.hip): bilinear resize (align_corners=False) of maps
 * [n][h][w] to T x T, THEN a Gaussian of sigma image pixels, as the one linear operator out = A_y M A_x^T, A = G R per axis.  R is
 * the [T][extent] bilinear matrix (src = max((dst + 0.5) extent / T - 0.5, 0), neighbour clamped); G the [T][T] Gaussian of radius
 * r = int(4 sigma + 0.5), taps exp(-0.5 (d / sigma)^2) normalised in float64, indices outside [0, T) folded back: border
 * 'symmetric' folds b a | a b (scipy.ndimage mode='reflect', what the PatchCore and PaDiM code runs), border 'reflect' folds
 * c b | a b c (torch / kornia reflect padding, what anomalib runs).  The caller builds A in float64 and passes each axis in band
 * form: first int32 [T] = the first source index of the row's run of non-zeros, weights fp32 [T][K] = A[d][first[d] .. + K)
 * rounded once, zero-padded, first[d] + K <= extent; K_y <= h, K_x <= w.  out [n][T][T] fp32: per pixel two chains of K FMAs in
 * ascending tap order -- the same bits whatever n and band.  band: output rows per workgroup, 0 = ssad_resize_gaussian_band(h, w,
 * T, Ky) (the largest of 32, 16, .. whose source rows and intermediate fit the LDS of a launch; 0 when none does).  A bad argument
 * (null pointer, a size or K below 1, a band that does not fit) returns 2 before any launch. */
int ssad_resize_gaussian_band(int h, int w, int T, int Ky);
int ssad_resize_gaussian(const float* maps, int64_t n, int h, int w, const int32_t* y_first, const float* y_weights, int Ky,
                         const int32_t* x_first, const float* x_weights, int Kx, int T, int band, float* out, void* stream);

/* ---- half-tensor forms of the precision-16 training step ----
 * pl.Trainer(precision=16) (src/self_supervised/tools.py:263, :296) runs the reference's training_step (models.py:256-277) under
 * torch.autocast(float16): every conv / linear / BatchNorm output of the trunk is an fp16 tensor in memory and so is its gradient.
 * The `_h` entry points below are the SAME kernels as their fp32-tensor namesakes with the activation tensors (void*: N H W C
 * halves) read and written as halves; arithmetic, BatchNorm statistics (those of the stored halves), parameters and parameter
 * gradients stay fp32.  Same call sites, same argument meaning. */
/* one rounded copy of the fp32 master arena per step (autocast's weight cast): src, dst 16-byte aligned */
int ssad_cvt_f32_f16(const float* src, void* dst, int64_t n, void* stream);
/* ssad_flip_transpose_batch writing halves (dgrad operands) */
int ssad_flip_transpose_batch_h(const float* src, void* dst, const int64_t* desc, int n, void* stream);
/* resnet.conv1 with fp16 operands, z stored as halves [B][Ho][Wo][64] (ssad_stem_fwd_stats16) */
int ssad_stem_fwd_stats16_h(const float* img, int B, int H, int W, const void* wk16, void* out, float eps, float momentum,
                            float* mean, float* invstd, float* running_mean, float* running_var, double* workspace, void* stream);
int ssad_bn_relu_maxpool_fwd_h(const void* z, const float* mean, const float* invstd, const float* gamma, const float* beta, void* out,
                               uint8_t* idx, int64_t N, int H, int W, int C, void* stream);
/* conv + train-mode BatchNorm statistics, dgrad: in / out / residual AND the weights (w_ohwi, w_flipT) are halves
 * (ssad_conv_igemm_fwd_stats with bf16 = 2, ssad_conv_igemm_dgrad_f16) */
int ssad_conv_igemm_fwd_stats_h(const void* in, const void* w_ohwi, void* out, int64_t N, int H, int W, int Cin, int Cout, int KH,
                                int KW, int stride, int pad, float eps, float momentum, float* mean, float* invstd,
                                float* running_mean, float* running_var, double* workspace, void* stream);
int ssad_conv_igemm_dgrad_h(const void* dy, const void* w_flipT, void* dx, const void* residual, int64_t N, int Hy, int Wy, int Cout,
                            int Hx, int Wx, int Cin, int KH, int KW, int stride, int pad, void* stream);
/* ssad_conv3x3_c64_op with op = 2 and in / out / residual / emit as halves (the weights are the fp32 OHWI master copy) */
int ssad_conv3x3_c64_h(const void* in, const float* w_ohwi, void* out, const void* residual, const float* tr_mean,
                       const float* tr_invstd, const float* tr_gamma, const float* tr_beta, void* emit, int64_t N, int H, int W,
                       double* stats_ws, float eps, float momentum, float* mean, float* invstd, float* running_mean,
                       float* running_var, void* stream);
int ssad_bn_stats_h(const void* z, int64_t R, int C, float eps, float momentum, float* mean, float* invstd, float* running_mean,
                    float* running_var, double* workspace, void* stream);
int ssad_bn_apply_fwd_h(const void* z, const float* mean, const float* invstd, const float* gamma, const float* beta,
                        const void* residual, void* y, int64_t R, int C, int relu, void* stream);
int ssad_gap_fwd_h(const void* in, float* out, int64_t N, int HW, int C, int out_stride, int out_offset, void* stream);
int ssad_gap_bwd_h(const float* dpooled, void* dy, int64_t N, int HW, int C, int stride, int offset, int accumulate, void* stream);
int ssad_bn_bwd_reduce_h(const void* dy, const void* yact, const void* z, const float* mean, const float* invstd, float* dbeta,
                         float* dgamma, int64_t R, int C, double* workspace, void* stream);
int ssad_bn_bwd_reduce_zmask_h(const void* dy, const void* z, const float* mean, const float* invstd, const float* gamma,
                               const float* beta, float* dbeta, float* dgamma, int64_t R, int C, double* workspace, void* stream);
int ssad_bn_apply_bwd_h(const void* dy, const void* yact, const void* z, const float* mean, const float* invstd, const float* gamma,
                        const float* dbeta, const float* dgamma, void* dz, void* dres, int64_t R, int C, int eval_mode, void* stream);
int ssad_bn_apply_bwd_zmask_h(const void* dy, const void* z, const float* mean, const float* invstd, const float* gamma,
                              const float* beta, const float* dbeta, const float* dgamma, void* dz, int64_t R, int C, void* stream);
int ssad_pool_bn_relu_bwd_h(const uint8_t* idx, const void* dpool, const void* z, const float* mean, const float* invstd,
                            const float* gamma, const float* beta, float* dbeta, float* dgamma, void* dz, int64_t N, int H, int W,
                            int C, int64_t dpool_elems, double* workspace, void* stream);
/* 3x3 / stride 1 / pad 1 convolution over half tensors (csrc/conv16.hip): the BasicBlock conv3x3 layers of the trunk (models.py:224
 * under pl.Trainer(precision=16)) forward and -- with the flipped filter -- their input gradients.  Halo-tile form with persistent
 * workgroups: the input tile of 64 channels is staged once for its nine taps, optionally through relu(bn(x)) of the producing layer
 * (tr_*: that layer's batch statistics and affine parameters; `emit` then receives the transformed activation for this layer's weight
 * gradient), weight slices two steps ahead, accumulators stored straight from registers.  w_ohwi: halves [Cout][3][3][Cin].
 * stats_ws: ssad_conv3x3_h_stats_rows(...) * 2 * Cout doubles -> mean / invstd / running statistics of the stored output. */
int ssad_conv3x3_h_ok(int Cin, int Cout);
int64_t ssad_conv3x3_h_stats_rows(int64_t N, int H, int W, int Cout);
int ssad_conv3x3_h(const void* in, const void* w_ohwi, void* out, const void* residual, const float* tr_mean, const float* tr_invstd,
                   const float* tr_gamma, const float* tr_beta, void* emit, int64_t N, int H, int W, int Cin, int Cout, double* stats_ws,
                   float eps, float momentum, float* mean, float* invstd, float* running_mean, float* running_var, void* stream);
/* The same convolution with the filter fed to the matrix cores from registers (csrc/conv16w.hip), for launches that fill the chip
 * (ssad_conv3x3_hw_ok: maps of 16 x 16 blocks or 8 x 8 maps, >= ~200 (tile, channel slab) pairs): a wave owns 128 pixels x 64 channels,
 * the filter is packed once per step in fragment order [Cout/32][tap][Cin/16][2][32][8] halves (ssad_conv3x3_hw_pack_batch, from the
 * fp32 master weights: desc[5 k ..] = source offset in floats, destination offset in halves, Cout, Cin of the conv that runs on it,
 * flip = 1 when the source is the OHWI filter [Cin][3][3][Cout] of the forward conv whose input gradient this is), the halo is staged
 * by four extra waves of the workgroup.  Arguments of ssad_conv3x3_hw as ssad_conv3x3_h, w_packed in place of w_ohwi, plus res_mask
 * (optional, with a residual; round 6): the residual is the identity-branch gradient (dy, nibble mask) of ssad_bn_apply_fwd_mask_h --
 * two mask bytes per 8-half piece -- applied while the residual is staged. */
int ssad_conv3x3_hw_ok(int64_t N, int H, int W, int Cin, int Cout);
int64_t ssad_conv3x3_hw_packed_size(int Cin, int Cout);
int64_t ssad_conv3x3_hw_stats_rows(int64_t N, int H, int W, int Cout);
int ssad_conv3x3_hw_pack_batch(const float* src, void* dst, const int64_t* desc, int n, void* stream);
int ssad_conv3x3_hw(const void* in, const void* w_packed, void* out, const void* residual, const uint8_t* res_mask, const float* tr_mean,
                    const float* tr_invstd, const float* tr_gamma, const float* tr_beta, void* emit, int64_t N, int H, int W, int Cin, int Cout,
                    double* stats_ws, float eps, float momentum, float* mean, float* invstd, float* running_mean, float* running_var,
                    void* stream);
/* The exact-fp32 instantiation of the same kernel (csrc/conv16w.hip, T = float: v_mfma_f32_32x32x2_f32; statistics: packed fp32 sums of 32 values per tile and column, added in
 * double across tiles):
 * the 3 x 3 / stride 1 convs of the fp32 training step (models.py:224) forward and -- with the flipped pack -- their input gradients,
 * whenever the launch fills the chip (ssad_conv3x3_fw_ok; other launches stay on ssad_conv3x3_c64 / ssad_conv_igemm_*).  The filter pack
 * holds floats in fragment order [Cout/32][tap][Cin/8][2][32][4]; res_mask: the residual is the identity-branch gradient (dy, nibble mask)
 * of ssad_bn_apply_fwd_mask, applied while the residual is staged. */
int ssad_conv3x3_fw_ok(int64_t N, int H, int W, int Cin, int Cout);
int ssad_conv3x3_fw_pack_batch(const float* src, float* dst, const int64_t* desc, int n, void* stream);
int ssad_conv3x3_fw(const float* in, const float* w_packed, float* out, const float* residual, const uint8_t* res_mask,
                    const float* tr_mean, const float* tr_invstd, const float* tr_gamma, const float* tr_beta, float* emit, int64_t N,
                    int H, int W, int Cin, int Cout, double* stats_ws, float eps, float momentum, float* mean, float* invstd,
                    float* running_mean, float* running_var, void* stream);
/* Inference form of ssad_conv3x3_fw (the layer1 convs of the patch-scoring pass, models.py:224 in eval mode, replacing ssad_conv3x3_c64_eval
 * on launches that fill the chip): out = act(conv(in) + shift (+ residual)); the folded BatchNorm's SCALE goes into the packed filter
 * (ssad_conv3x3_fw_pack_scaled: w[o][..] * scale[o], fragment order), its shift is added in the epilogue, the residual (NHWC) by the matrix
 * cores.  16 x 16 maps of 64 channels run two maps per tile.  out_hwnc: output written position-major [H][W][N][C]. */
int ssad_conv3x3_fw_eval_ok(int64_t N, int H, int W, int Cin, int Cout);
int ssad_conv3x3_fw_pack_scaled(const float* w_ohwi, const float* scale, float* dst, int Cout, int Cin, void* stream);
int ssad_conv3x3_fw_eval(const float* in, const float* w_packed, float* out, const float* shift, const float* residual, int relu, int64_t N,
                         int H, int W, int Cin, int Cout, int out_hwnc, void* stream);
/* Weight gradient of the 3 x 3 / pad 1 convolutions, stride 1 AND 2, over half tensors (csrc/wgrad16.hip): tiles go to LDS as they lie
 * in memory and the [pixel][channel] -> [channel][pixel] transpose the matrix instruction needs happens in the fragment reads (eight
 * 2-byte LDS reads per operand), so no staging waves, no conversion; same slab contract as ssad_conv_wgrad3x3_halo16:
 * splits = ssad_wgrad3x3_g16_splits(N, Ho, Wo, Cin, Cout, stride), then ssad_wgrad_reduce(slab, dw, splits, Cout, 9 * Cin, 3, 3, Cin, ..).
 * Replaces the conv2d weight-gradient node of every BasicBlock conv3x3 under pl.Trainer(precision=16) (tools.py:263, :270, :303). */
int ssad_wgrad3x3_g16_ok(int Cin, int Cout, int KH, int KW, int stride, int pad);
int ssad_wgrad3x3_g16_splits(int64_t N, int Ho, int Wo, int Cin, int Cout, int stride);
int ssad_conv_wgrad3x3_g16_h(const void* dz, const void* x, float* slab, int splits, int64_t N, int Ho, int Wo, int H, int W, int Cin,
                             int Cout, int stride, int64_t dz_elems, void* stream);
/* weight gradients from half tensors (fp32 slabs, then ssad_wgrad_reduce, as the fp32-tensor forms) */
int ssad_conv_wgrad3x3_halo16_h(const void* dz, const void* x, float* slab, int splits, int64_t N, int H, int W, int Cin, int Cout,
                                int64_t dz_elems, void* stream);
int ssad_conv_wgrad_f16_h(const void* dy, const void* x, float* slab, int splits, int64_t N, int H, int W, int Cin, int Cout, int KH,
                          int KW, int stride, int pad, int64_t dy_elems, void* stream);
int ssad_stem_wgrad_h(const float* img, const void* dz, float* dw, int B, int H, int W, int64_t dz_elems, int to_oihw, int accumulate,
                      float* workspace, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SSAD_H */
