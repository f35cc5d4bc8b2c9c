/* osk.h — C ABI of libosk_hip.so: the MI355X (gfx950) kernels of the Open-Sora denoise path.
 *
 * The reference (hpcaitech/Open-Sora v2.0, /root/reference) has no native code and no FFI: every GPU
 * kernel on its hot path is imported from a pip dependency (flash-attn, liger-kernel, cuBLAS/cuDNN via
 * torch).  Each entry point below therefore cites the reference *call site* whose arithmetic it replaces
 * (paths relative to /root/reference).  INTEGRATION.md shows the ctypes binding a reference maintainer
 * would add (it is the binding open_sora_amd/_C.py uses).
 *
 * Conventions
 *  - Plain pointers and sizes only; no torch types.  All pointers are DEVICE pointers unless noted.
 *  - `stream` is a hipStream_t passed as void*.  Every function only ENQUEUES work on `stream`:
 *    no allocation, no synchronisation, no global state in any compute entry point -> safe under hipGraph capture.
 *    (The only process-wide state are the two TOOL switches osk_gemm_tile_override / osk_attention_rows_override -- A/B timing aids
 *    that default to "by estimate" and are never set by the product path.)
 *  - bf16 tensors are passed as `const void*` / `void*` (16-bit storage); f32 as float*.
 *  - Strides are in ELEMENTS of the tensor's dtype.  "rows_per_batch" addressing: logical row m of a
 *    [B*L, ...] matrix lives at  base + (m / L) * batch_stride + (m % L) * row_stride, so that streams
 *    stored inside larger joint buffers need no copies.
 *  - Return value: 0 = OSK_OK, <0 = invalid argument / unsupported shape (nothing was launched),
 *    >0 = hipError_t from the launch.
 */
#ifndef OSK_H
#define OSK_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* (osk_attention_fwd_ragged_bf16 / osk_attention_ragged_workspace_bytes / osk_attention_merge_into_bf16 -- sequence parallelism over
 * token counts the rank count does not divide -- are additive entries too: the version stays 2, as the suite pins it.)
 * (osk_attention_merge_bf16 was added the same way: a new entry, no existing contract changed.)
 * (round 6 added osk_gemm_group_bf16 without changing any existing contract: the version stays 2.)
 * 2 (round 5): osk_copy_rows_bf16 added; and the contracts that changed under version 1 during round 4 are now versioned -- the
 * key order osk_v_transpose_bf16 bakes into V^T for head_dim 64 (the 16x16x32 order of head_dim 72: attention_fwd.hip), the entry
 * points osk_gemm_geglu_bf16 / osk_attention_short_bf16 / osk_attention_hd512_fwd_ws_bf16 / osk_causal_conv3d_gnin_ndhwc_bf16.
 * A binding must refuse a library whose version it was not written for (open_sora_amd/_C.py does). */
#define OSK_ABI_VERSION 2
int osk_abi_version(void);
/* name of the arch the library was compiled for ("gfx950") — host-only, no GPU needed */
const char* osk_arch(void);

/* ---- LayerNorm(no affine, eps) + adaLN modulate:  out = (1 + scale[b]) * LN(x) + shift[b]
 * replaces nn.LayerNorm + the bf16 elementwise chain at opensora/models/mmdit/layers.py:205-206,
 * 223-224, 248, 252, 311-312 and LastLayer layers.py:400.  x/out bf16 [B*L, D]; shift/scale f32,
 * element (b, d) at ptr[b * mod_batch_stride + d].  Statistics and modulate in f32, one rounding. */
int osk_ln_modulate_bf16(const void* x, int64_t x_batch_stride, int64_t x_row_stride,
                         void* out, int64_t out_batch_stride, int64_t out_row_stride,
                         const float* shift, const float* scale, int64_t mod_batch_stride,
                         int B, int L, int D, float eps, void* stream);

/* ---- C = epilogue(A @ W^T + bias) on MFMA bf16 (f32 accumulate).
 * replaces every nn.Linear on the path: layers.py:146-152,209-215,226-232,247-252,314-320,332-333,
 * 401; model.py:176-180,191.  A bf16 [M, K] (rows_per_batch addressing), W bf16 [N, K] row-major
 * (nn.Linear.weight layout), bias f32 [N] or NULL.
 * Epilogue, in f32, in this order:
 *   v = acc + bias[n];  if (n >= gelu_from) v = gelu_tanh(v);
 *   if (gate) v = res[m, n] + gate[b * gate_batch_stride + n] * v;      (res bf16, same addressing as C)
 *   C[m, n] = bf16(v)            (or f32 when out_f32 != 0)
 * K % 64 == 0 required; any M, N >= 1.  gelu_from = N disables GELU.  res may alias C. */
int osk_gemm_bf16(const void* A, int64_t a_batch_stride, int64_t a_row_stride, int a_rows_per_batch,
                  const void* W, int64_t w_row_stride, const float* bias,
                  void* C, int64_t c_batch_stride, int64_t c_row_stride, int c_rows_per_batch,
                  const void* res, const float* gate, int64_t gate_batch_stride,
                  int M, int N, int K, int gelu_from, int out_f32, void* stream);

/* reporting / tools: the tile kernel osk_gemm_bf16 picks for an [M, N, K] problem whose operands the large tiles support -- 2 = 256 x 256
 * (gemm256x_kernel), 1 = 256 x 128 (gemm256p_kernel), 0 = 128 x 128 (gemm_bf16_kernel) -- by estimated rounds of the chip x per-tile rate;
 * osk_gemm_tile_override(kind) forces one of them process-wide for same-process A/B timing (tools/gemm_tile_ab.py; -1 = back to the estimate;
 * never set in production code). */
int osk_gemm_tile_choice(int M, int N, int K);
int osk_gemm_tile_override(int tile_kind);
/* ... and the kernel osk_gemm_bf16 launches for operands with THESE strides (elements), from the dispatch's own code: the estimate's
 * choice where the large tiles take the operands, 0 otherwise.  The large tiles address every tile relative to its own origin: what
 * has to fit their 32-bit lane offsets is each 256-row window of A and of W (2^32 - 1 bytes from the window's lowest row, a batch
 * jump inside the window included) -- not the operand, which may span more than 4 GiB.  < 0: invalid arguments. */
int osk_gemm_tile_choice_strided(int M, int N, int K, int64_t a_batch_stride, int64_t a_row_stride, int a_rows_per_batch,
                                 int64_t w_row_stride);

/* ---- TWO Linear layers that differ only in their operands and row count in ONE launch.
 * replaces the img-stream / txt-stream pairs of DoubleStreamBlockProcessor (layers.py:209-215 img_attn.qkv | txt_attn.qkv,
 * 247 img_attn.proj | 251 txt_attn.proj, 248 img_mlp | 252 txt_mlp): same N, K and epilogue kind, separate weights, inputs and
 * outputs.  Exactly osk_gemm_bf16(first...) followed by osk_gemm_bf16(second...) with out_f32 = 0 (the two must not depend on
 * each other); where both problems take the 256 x 256 tile kernel they are walked as one tile list, so the small text GEMM
 * (a third of the chip for one round when launched alone) fills the last round of the image GEMM. */
typedef struct OskGemmOperands {
  const void* A; int64_t a_batch_stride, a_row_stride; int a_rows_per_batch;
  const void* W; int64_t w_row_stride; const float* bias;
  void* C; int64_t c_batch_stride, c_row_stride; int c_rows_per_batch;
  const void* res; const float* gate; int64_t gate_batch_stride;
  int M;
} OskGemmOperands;
int osk_gemm_bf16_pair(const OskGemmOperands* first, const OskGemmOperands* second, int N, int K, int gelu_from, void* stream);

/* ---- a GROUP of up to four Linear problems that share K (at most two plain + two V^T tasks) on the 256 x 256 tile kernel (round 6).
 * replaces, per block, the QKV projection + the V re-layout of the reference's attention path: layers.py:209-220 (img / txt qkv
 * Linear + rearrange), :314-320 (linear1 + split + rearrange), math.py:22-36 (attention() permutes V to the kernel's layout) --
 * the V columns of the projection are written DIRECTLY as the key-major V^T operand of osk_attention_fwd_*_bf16, so the separate
 * osk_v_transpose_bf16 pass (read + write of V per block) disappears.  The plain tasks go out as one launch (two of equal N: one tile
 * list, the small text-stream problem fills the image problem's last round), the V^T tasks as one launch of the kernel's V^T form.
 * Plain task (vt_head_dim == 0): exactly osk_gemm_bf16(op..., N, K, gelu_from, out_f32 = 0), except that the physical columns
 *   [skip_from, skip_from + skip_len) of W / bias / C are neither computed nor stored (skip_len == 0: none; skip_from % 256 == 0,
 *   skip_len % 8 == 0, no gate): a single-stream block's linear1 without its V columns -- row layout [q | k | . | mlp].
 * V^T task (vt_head_dim = 64 / 72 / 128): op.A = the activations X bf16 [op.M = B * L rows, K] (rows_per_batch addressing,
 *   a_rows_per_batch = L), op.W = W_v bf16 [N = H * hd, K], op.bias = b_v f32 [N] | NULL, op.C = V^T base pointer (bf16),
 *   c_batch_stride = elements between batch items, c_row_stride = elements between (head, dim) rows (>= round_up(L, 64));
 *   res / gate NULL; gelu_from / skip_* ignored:
 *     C[b * c_batch_stride + n * c_row_stride + p] = bf16(sum_k X[b, key(p), k] W_v[n, k] + b_v[n])   for key(p) < L,  else 0,
 *   p < round_up(L, 64), key(p) = the position -> key map of osk_v_transpose_bf16 for this head_dim (inside every 64-key group) --
 *   i.e. the result of osk_gemm_bf16 into a [B, L, N] tensor followed by osk_v_transpose_bf16, with the same f32 accumulation
 *   and ONE rounding (the bias is added after the K loop instead of initialising the accumulators: results may differ from the
 *   two-kernel path in the last bf16 bit).  A stream stored behind another one on the key axis (img behind txt) passes
 *   C + its first position (a multiple of 64).
 * All tasks must qualify for the 256 x 256 tile kernel (M >= 256, N >= 128 (V^T: H * hd >= 256), every 256-row window of the
 * operands within 2^32 - 1 bytes of its own origin -- osk_gemm_tile_choice_strided; the operands may span more than 4 GiB):
 * otherwise OSK_EUNSUPPORTED is returned and NOTHING is launched (the caller runs the single calls). */
typedef struct OskGemmTask {
  OskGemmOperands op;
  int N, gelu_from;
  int skip_from, skip_len;
  int vt_head_dim;
} OskGemmTask;
int osk_gemm_group_bf16(const OskGemmTask* tasks, int n_tasks, int K, void* stream);

/* ---- GEGLU up-projection (the STDiT-generation block's "GEGLU MLP" of BASELINE.json's
 * north_star; the mounted v2.0 reference has no GEGLU call site -- its MLP is Linear -> GELU(tanh) -> Linear, layers.py:277-281 --
 * so this entry is PARITY-UNPINNED: semantics = diffusers' FeedForward(activation_fn="geglu") EXCEPT the activation: diffusers'
 * GEGLU applies the exact (erf) F.gelu to the gate, this entry the tanh approximation the v2.0 blocks use everywhere
 * (|gelu_tanh - gelu_erf| <= ~1e-3 absolute, a systematic difference a checkpoint trained with diffusers GEGLU would see per MLP;
 * the fp64 test oracle uses the same tanh formula, so it does not measure this deviation -- an erf epilogue is one more class):
 *   C[m, j] = (A W_v^T + b_v)[m, j] * gelu_tanh((A W_g^T + b_g)[m, j]),   j < N_out
 * as ONE GEMM with N = 2 N_out whose epilogue multiplies value and gate in registers.  W_packed [2 N_out, K] / bias_packed
 * [2 N_out]: value and gate rows interleaved in blocks of 16 -- packed row 32 j2 + i (i < 16) = value row 16 j2 + i, packed row
 * 32 j2 + 16 + i = gate row 16 j2 + i (open_sora_amd/_C.py::geglu_pack builds it once at plan time); N_out % 16 == 0.
 * Shapes the 256 x 256 tile kernel does not take (M < 256, narrow N, ...) run the plain GEMM into `workspace` (>= M * 2 N_out * 2
 * bytes, 16-byte aligned) followed by a row kernel; without a workspace they return OSK_EUNSUPPORTED and launch nothing. */
int osk_gemm_geglu_bf16(const void* A, int64_t a_batch_stride, int64_t a_row_stride, int a_rows_per_batch,
                        const void* W_packed, int64_t w_row_stride, const float* bias_packed, void* C,
                        int64_t c_batch_stride, int64_t c_row_stride, int c_rows_per_batch, int M, int N_out, int K,
                        void* workspace, int64_t workspace_bytes, void* stream);

/* ---- FP8 (OCP e4m3fn) variant of the Linear GEMM: BASELINE configs[4] ("fp8 MFMA"); the reference itself runs its
 * nn.Linear layers (same call sites as osk_gemm_bf16) in bf16, so this is an opt-in mode.
 * osk_quantize_rows_fp8: dynamic per-row quantisation of a bf16 [M, K] activation (rows_per_batch addressing):
 *   scales[m] = absmax(x[m, :]) / 448  (1.0 for an all-zero row),  out8[m, k] = e4m3(clamp(x[m, k] * (448 / absmax)))
 *   out8 is contiguous [M, K] bytes.  K % 8 == 0.  Also used once per weight matrix at load time.
 * osk_gemm_fp8: C = epilogue(a_scale[m] * w_scale[n] * (A8 @ W8^T) + bias), the epilogue of osk_gemm_bf16, on
 *   v_mfma_f32_32x32x64_f8f6f4 (f32 accumulate).  Strides of A8 / W8 in bytes, multiples of 16; K % 128 == 0,
 *   M >= 256, N >= 128, every 256-row window of A8 / W8 within 2^32 - 1 bytes of its own origin (the operands may span more than
 *   4 GiB); returns OSK_EUNSUPPORTED (-2) otherwise: such layers stay on osk_gemm_bf16. */
/* osk_ln_modulate_fp8: osk_ln_modulate_bf16 followed by osk_quantize_rows_fp8 in one pass (bit-identical to the pair:
 * the modulated row is rounded to bf16 first): out8 = e4m3 bytes [B*L, D] contiguous, scales f32 [B*L]. */
int osk_ln_modulate_fp8(const void* x, int64_t x_batch_stride, int64_t x_row_stride, void* out8, float* scales,
                        const float* shift, const float* scale, int64_t mod_batch_stride,
                        int B, int L, int D, float eps, void* stream);
int osk_quantize_rows_fp8(const void* x, int64_t x_batch_stride, int64_t x_row_stride, int rows_per_batch,
                          void* out8, float* scales, int M, int K, void* stream);
int osk_gemm_fp8(const void* A8, int64_t a_batch_stride, int64_t a_row_stride, int a_rows_per_batch,
                 const float* a_scale, const void* W8, int64_t w_row_stride, const float* w_scale,
                 const float* bias, void* C, int64_t c_batch_stride, int64_t c_row_stride, int c_rows_per_batch,
                 const void* res, const float* gate, int64_t gate_batch_stride,
                 int M, int N, int K, int gelu_from, int out_f32, void* stream);

/* ---- skinny matrix-vector batch (any Bv; launched in slices of <= 8 rows, K <= 16384):
 * out[b, n] (+)= act_in(x[b, :]) . W[n, :] + bias[n]
 * replaces Modulation (layers.py:184-191), MLPEmbedder (layers.py:91-99) and LastLayer.adaLN_modulation
 * (layers.py:396,399): weight-bandwidth bound.  One launch covers a LIST of layers that share x:
 * descriptor arrays (device memory, n_tasks entries each, one task = up to 64 consecutive rows of one
 * layer):  w_ptrs[i] -> bf16 W rows [rows, K];  b_ptrs[i] -> bf16 bias or 0;  out_cols[i] = column
 * offset in out;  n_rows[i].  x f32 [Bv, K], out f32 [Bv, out_batch_stride].
 * act_in: 0 none, 1 SiLU.  accumulate != 0 adds into out. */
int osk_gemv_tasks_bf16(const float* x, int64_t x_batch_stride, int Bv, int K,
                        const uint64_t* w_ptrs, const uint64_t* b_ptrs, const int32_t* out_cols,
                        const int32_t* n_rows, int n_tasks,
                        float* out, int64_t out_batch_stride, int act_in, int accumulate, void* stream);

/* ---- sinusoidal timestep embedding: out[b] = [cos(a) | sin(a)], a = time_factor * t[b] * exp(-ln(max_period) i / half)
 * replaces timestep_embedding, layers.py:68-88 (f32). */
int osk_timestep_embedding(const float* t, int B, int dim, float max_period, float time_factor,
                           float* out, void* stream);

/* ---- RoPE angle tables from integer (t, h, w) position ids.
 * replaces EmbedND / rope (layers.py:31-44, math.py:50-57; f64 angles) and LigerEmbedND / liger_rope
 * (layers.py:47-65, math.py:39-47; f32 angles).  ids f32 [n_rows, n_axes]; axes_dim[n_axes] host ints;
 * cos/sin f32 [n_rows, sum(axes_dim)/2] with pair index j ordered axis-major.  f32_angles selects the
 * liger arithmetic. */
int osk_rope_table(const float* ids, int64_t n_rows, int n_axes, const int32_t* axes_dim_host,
                   double theta, int f32_angles, float* cos_out, float* sin_out, void* stream);

/* ---- per-head RMSNorm (QK-norm) + RoPE on q and k, in place, inside a [B, L, ld] projection buffer.
 * replaces QKNorm/FusedRMSNorm (layers.py:114-135 -> liger RMSNorm "llama") followed by apply_rope
 * (math.py:60-65, rope_mode 0 = interleaved pairs (2j,2j+1)) or LigerRopeFunction (math.py:27,
 * rope_mode 1 = half-split pairs (j, j+hd/2)).
 * q row (b,l) head h at q + b*batch_stride + l*row_stride + h*hd (same for k).  Rows l < l_split use
 * (q_scale0,k_scale0) (the txt stream's norm weights), rows >= l_split use (q_scale1,k_scale1).
 * Scales bf16 [hd].  cos/sin f32 [*, L, hd/2] with batch stride cs_batch_stride (0 = shared).
 * Rounding points follow the reference: bf16(x*rrms) * bf16 scale -> bf16, rotate in f32, -> bf16.
 * Either q or k (not both) may be NULL: only the other one is processed (the sequence-parallel path norms
 * K first so its all-gather can start while the Q / MLP projections run).
 * q_mult multiplies the rotated q (not k) in f32 BEFORE its final rounding to bf16: pass 1.0 for the reference's
 * values, or softmax_scale * log2(e) together with q_prescaled = 1 in osk_attention_fwd_bf16 (the reference
 * multiplies the f32 scores by the scale after q.k; folding it into q's single rounding keeps the same
 * one-rounding error on q and lets the attention kernel exponentiate the MFMA output directly). */
int osk_qknorm_rope_bf16(void* q, void* k, int64_t batch_stride, int64_t row_stride,
                         const void* q_scale0, const void* k_scale0,
                         const void* q_scale1, const void* k_scale1, int l_split,
                         const float* cos_t, const float* sin_t, int64_t cs_batch_stride,
                         int B, int L, int H, int hd, int rope_mode, float eps, float q_mult, void* stream);

/* ---- V -> key-major transposed copy for the attention kernel's PV operand.
 * (internal layout, no reference counterpart: flash-attn does this transpose in shared memory.)
 * v row (b,l) head h at v + b*batch_stride + l*row_stride + h*hd.
 * vt [B, H, hd, Lp], Lp = round_up(L, 64), zero-filled for keys >= L.  The key order inside a 64-key tile is the one in
 * which the attention kernel of that head_dim holds P for its second product (an internal contract between the two calls):
 *   hd 128 (P.V on 32x32x16 MFMAs): inside every group of 16 keys the two middle quads are swapped (k0-3, k8-11, k4-7,
 *     k12-15) -- the order the score accumulators hand P back, no cross-lane shuffle;
 *   hd 72 and hd 64 (the same loop; P.V on 16x16x32 MFMAs, 80 instead of 96 padded rows): 16-byte chunk c of a tile row = 32-key half c / 4, MFMA
 *     lane row c % 4, holding keys {0-3, 8-11}, {16-19, 24-27}, {4-7, 12-15}, {20-23, 28-31} of that half for rows 0..3. */
int osk_v_transpose_bf16(const void* v, int64_t batch_stride, int64_t row_stride,
                         void* vt, int B, int L, int H, int hd, void* stream);

/* ---- gathered K / V segments -> the operands of ONE key segment (an additive entry, the version stays 2).
 * It stands beside the KV exchange around attention of opensora/models/mmdit/distributed.py (ring hops + LSE merge :223-313,
 * Ulysses all-to-all :473-495) and replaces nothing there: the reference never re-lays its exchanged K / V out.  Here the exchange
 * buffers of open_sora_amd/seqpar.py are segment-major, and osk_attention_fwd_window_bf16 takes one key segment; this call turns
 * the one into the other in a single HBM-bound launch (K and V each read once and written once).
 * k_seg, v_seg: key j < L of batch b, head h lives in segment s = j / seg_len, row r = j % seg_len, at
 *   base + s*seg_stride + b*batch_stride + r*row_stride + h*hd (elements; the strides are shared by K and V).
 *   (n_seg - 1)*seg_len < L <= n_seg*seg_len: the last segment may be short; its rows >= L - (n_seg - 1)*seg_len are never read.
 * k_out: k_out[b, j, :] = that K row for j < L -- a [B, L, H*hd] view, batches ko_batch_stride and rows ko_row_stride elements apart.
 * vt_out: [B, H, hd, round_up(L, 64)] contiguous, bit-identical to what osk_v_transpose_bf16 writes for the contiguous [B, L, H*hd]
 *   V of the same keys: the key order inside each 64-key tile documented above, zeros for keys >= L.
 * OSK_EINVAL: L / n_seg / seg_len outside the rule above, B or H <= 0, a NULL pointer or one not 16-byte aligned, a stride that is
 * no multiple of 8.  hd in {64, 72, 128} (else OSK_EUNSUPPORTED).  A refused call launches nothing.
 * No allocation, no memset, no atomics on global memory, no host synchronisation: capturable in a hipGraph. */
int osk_kv_join_bf16(const void* k_seg, const void* v_seg,
                     int64_t seg_stride, int64_t batch_stride, int64_t row_stride,   /* elements, shared by K and V */
                     void* k_out, int64_t ko_batch_stride, int64_t ko_row_stride,
                     void* vt_out,
                     int B, int H, int hd, int n_seg, int seg_len, int L, void* stream);

/* ---- the e4m3 counterparts of the join, for frame-window attention under sequence parallelism in fp8 mode (additive entries, the
 * version stays 2).  The operands the fp8 kernels consume as e4m3 travel as e4m3, token-major, at one byte per element; the join
 * lays the gathered segments out as the operands of one key segment.  Nothing in the reference corresponds to either.
 *
 * osk_kv_quant_rows_fp8: x bf16 [B, L, H*hd] view (batch / row strides in elements, multiples of 8; 16-byte aligned pointer; last
 *   dim contiguous), scales f32 [B, H] -> out, e4m3 bytes [B, L, H*hd] token-major with batch / row strides of its own in BYTES (a
 *   rank's slot of a gather buffer): out[b, l, h*hd + d] = e4m3(clamp(x[b, l, h*hd + d] / scales[b, h], -448, 448)) -- the IEEE f32
 *   division, the clamp and the v_cvt_pk_fp8_f32 rounding of osk_k_pack_fp8 / osk_v_transpose_fp8, so every byte is the one those
 *   calls produce for the same element and scale.  hd 128: 16-byte stores (out 16-byte aligned, its strides multiples of 16);
 *   hd 72: a head of 72 bytes is no multiple of 16, so 8-byte stores (out 8-byte aligned, its strides multiples of 8).  Any other
 *   hd: OSK_EUNSUPPORTED.  OSK_EINVAL: a NULL pointer, a pointer or stride off the alignment above, B, H or L <= 0 (or B, H > 65535).
 *
 * osk_kv_join_fp8: the gathered segments (key j < L in segment s = j / seg_len, row r = j % seg_len; (n_seg - 1)*seg_len < L <=
 *   n_seg*seg_len; the rows of a short last segment behind key L - 1 are never read) -> the operands of one key segment of L keys:
 *   v_seg: e4m3 bytes at v_seg + s*v_seg_stride + b*v_batch_stride + r*v_row_stride + h*hd (bytes; hd 128: multiples of 16 and a
 *     16-byte aligned pointer, hd 72: multiples of 8 and an 8-byte aligned pointer) -> vt8_out [B, H, vt8_rows(hd), round_up(L, 64)],
 *     bit for bit what osk_v_transpose_fp8 writes for the contiguous V of the same keys with the scales the bytes were quantised
 *     with: the key order inside each 64-key tile, the ones / key-validity row (0x38 for keys < L, 0 behind them), the zero rows.
 *   k_kind OSK_KV_JOIN_K_E4M3 (hd 128 only, else OSK_EUNSUPPORTED): k_seg e4m3 bytes, strides in bytes (multiples of 16) ->
 *     k_out = k8 [B, H, round_up(L, 64), 128] contiguous, bit for bit what osk_k_pack_fp8 writes: rows L .. Lp-1 repeat row L-1.
 *     ko_batch_stride / ko_row_stride are not used.
 *   k_kind OSK_KV_JOIN_K_BF16 (K stays bf16: pv8): k_seg bf16, strides in elements (multiples of 8) -> k_out the [B, L, H*hd] bf16
 *     view of osk_kv_join_bf16 (ko strides in elements, multiples of 8).
 *   k_seg, k_out and vt8_out 16-byte aligned.  The argument checks are those of osk_kv_join_bf16 (OSK_EINVAL; a k_kind other than
 *   the two: OSK_EINVAL); hd in {72, 128}, else OSK_EUNSUPPORTED.  A refused call launches nothing.
 * Every byte of the outputs, key padding included, is written by the launch: nothing relies on a zeroed buffer.  No allocation, no
 * memset, no atomics on global memory, no host synchronisation: both are capturable in a hipGraph. */
#define OSK_KV_JOIN_K_BF16 0
#define OSK_KV_JOIN_K_E4M3 1
int osk_kv_quant_rows_fp8(const void* x, int64_t batch_stride, int64_t row_stride, const float* scales,
                          void* out, int64_t o_batch_stride, int64_t o_row_stride,      /* bytes */
                          int B, int L, int H, int hd, void* stream);
int osk_kv_join_fp8(const void* k_seg, int64_t k_seg_stride, int64_t k_batch_stride, int64_t k_row_stride, int k_kind,
                    const void* v_seg, int64_t v_seg_stride, int64_t v_batch_stride, int64_t v_row_stride,
                    void* k_out, int64_t ko_batch_stride, int64_t ko_row_stride,
                    void* vt8_out,
                    int B, int H, int hd, int n_seg, int seg_len, int L, void* stream);

/* ---- flash attention forward, non-causal: out = softmax(q k^T * scale) v, bf16 I/O, f32 softmax.
 * replaces flash_attn_func (math.py:16-19,33) and _flash_attn_forward with LSE
 * (distributed.py:148-161).
 * q  row (b,i) head h at q + b*q_batch_stride + i*q_row_stride + h*hd           (i < Lq)
 * k  key j lives in segment s = j / seg_len, r = j % seg_len (sequence-parallel all-gather layout;
 *    n_seg = 1, seg_len = Lk for one GPU): k + s*k_seg_stride + b*k_batch_stride + r*k_row_stride + h*hd
 * vt as written by osk_v_transpose_bf16 per segment: vt + s*vt_seg_stride + ((b*H + h)*hd + d)*seg_lp + r'
 *    with seg_lp = round_up(seg_len, 64).
 * out row (b,i) head h at out + b*o_batch_stride + i*o_row_stride + h*hd (may alias the dead v slot).
 * lse f32 [B, H, Lq] (natural log of the softmax denominator incl. scale) or NULL.
 * q_prescaled != 0: q already carries scale * log2(e) (osk_qknorm_rope_bf16's q_mult) and `scale` is ignored;
 * q_prescaled == 0: the kernel applies `scale` itself (the head_dim-72 hand-scheduled kernel then re-rounds
 * scale*log2(e)*q to bf16 once per workgroup: one extra bf16 rounding of q).
 * kv_batches: 0 (or B) = every query batch has its own keys; otherwise query batch b attends to key/value batch
 * b % kv_batches (head-parallel sequence parallelism: the B * P received query chunks share B key sets).
 * hd in {64, 72, 128}. */
int osk_attention_fwd_bf16(const void* q, int64_t q_batch_stride, int64_t q_row_stride,
                           const void* k, int64_t k_seg_stride, int64_t k_batch_stride, int64_t k_row_stride,
                           const void* vt, int64_t vt_seg_stride,
                           void* out, int64_t o_batch_stride, int64_t o_row_stride,
                           float* lse, int B, int H, int Lq, int n_seg, int seg_len, int hd,
                           float scale, int q_prescaled, int kv_batches, void* stream);

/* The same call with a caller-owned workspace (16-byte aligned, osk_attention_workspace_bytes() is always enough).
 * A workgroup owns a CU for its whole key loop, so a launch takes ceil(units / CUs) rounds; with a workspace the
 * work units of the last, partial round are cut into up to 8 key parts (whole key segments when n_seg > 1, runs of
 * 64-key tiles otherwise) that fill the idle CUs, and a small merge kernel combines the parts by their LSE
 * (head_dim 72 / 128; other head dims and workspace == NULL: exactly osk_attention_fwd_bf16).  Partials are kept in
 * f32 and rounded to bf16 once; a split row differs from the unsplit one only through the bf16 rounding of P against
 * the reference max of its own key part (same error bound against the exact result). */
int64_t osk_attention_workspace_bytes(void);
/* reporting / tests: the number of key parts (1 = no split) osk_attention_fwd_ws_bf16 -- a call WITHOUT a score bound -- would use */
int osk_attention_tail_split_factor(int B, int H, int Lq, int n_seg, int seg_len, int hd, int64_t workspace_bytes);
/* reporting / tests (round 5): the launch shape of osk_attention_fwd_bounded_bf16 for these arguments, from the selection code the
 * call itself runs: returns the number of key parts of the last round's work units and stores the query rows per work unit (256,
 * or 512 = the wide head_dim 72 / 64 layout, chosen by estimated rounds of the chip -- few batch x head pairs keep 256). */
int osk_attention_launch_shape(int B, int H, int Lq, int n_seg, int seg_len, int hd, float score_bound,
                               int64_t workspace_bytes, int* rows_per_unit);
/* tools only: force the work-unit rows of bounded head_dim 72 / 64 calls process-wide (256, or 512 where the wide layout is legal) for
 * same-process A/B timing (tools/attn_layout_ab.py); 0 = back to the estimate.  Never set in production code. */
int osk_attention_rows_override(int rows_per_unit);
int osk_attention_fwd_ws_bf16(const void* q, int64_t q_batch_stride, int64_t q_row_stride,
                           const void* k, int64_t k_seg_stride, int64_t k_batch_stride, int64_t k_row_stride,
                           const void* vt, int64_t vt_seg_stride,
                           void* out, int64_t o_batch_stride, int64_t o_row_stride,
                           float* lse, int B, int H, int Lq, int n_seg, int seg_len, int hd,
                           float scale, int q_prescaled, int kv_batches, void* workspace, int64_t workspace_bytes, void* stream);

/* The same call with a caller-supplied BOUND on the scores: |scale * log2(e) * q . k| <= score_bound for every (query, key) of
 * the launch (log2 units; with q_prescaled the bound is on q . k as stored).  The denoiser knows one for free: q and k come out
 * of an RMS norm (layers.py:102-135), so |q| <= sqrt(hd) max|w_q| and |k| <= sqrt(hd) max|w_k| (RoPE is a rotation).  With a bound
 * in (0, 56], n_seg == 1 and seg_len % 64 == 0 the head_dim-72 / 128 kernels run their FAST body: the online-softmax reference
 * is the constant bound instead of a tracked maximum (P = exp2(s - bound) can neither overflow nor vanish), which removes the
 * per-tile max chains, the rescale path and the segment / ragged-tile bookkeeping from the issue-bound loop.  The result is the
 * same softmax (a different, equally valid reference point: same error bound against the exact result).  score_bound == 0, or
 * any call shape outside the above: exactly osk_attention_fwd_ws_bf16.  A bound that is violated is the caller's bug: scores
 * above it by more than ~100 overflow. */
int osk_attention_fwd_bounded_bf16(const void* q, int64_t q_batch_stride, int64_t q_row_stride,
                           const void* k, int64_t k_seg_stride, int64_t k_batch_stride, int64_t k_row_stride,
                           const void* vt, int64_t vt_seg_stride,
                           void* out, int64_t o_batch_stride, int64_t o_row_stride,
                           float* lse, int B, int H, int Lq, int n_seg, int seg_len, int hd,
                           float scale, int q_prescaled, int kv_batches, float score_bound,
                           void* workspace, int64_t workspace_bytes, void* stream);

/* ---- the bound taken from the OPERANDS, on the device (round 6).  The weight-derived bound above is sqrt(hd)-loose per side: a
 * checkpoint whose QK-norm scale vectors (layers.py:102-135) have a few large entries exceeds 56 on paper while its actual q / k rows
 * stay far below -- and without a bound the step falls to the slower general body.  Here the caller passes NO promise:
 * osk_rownorm2_max_bf16: out[b * H + h] = max over rows l of sum_d x[b, l, h, d]^2 of a bf16 [B, L, H * hd] view (f32, device
 *   memory; one read of the tensor; accumulate != 0 folds into the values already there -- several key segments, or ranks
 *   that max-reduce afterwards).  Run it on the q and on the k the attention call receives.
 * osk_attention_fwd_auto_bf16: osk_attention_fwd_ws_bf16 on q_prescaled operands (q carries scale * log2 e: the norms must be those
 *   of the values the MFMA multiplies), q_norm2_max f32 [B, H], k_norm2_max f32 [kv_batches or B, H].  Every work unit derives its
 *   own bound sqrt(q_norm2_max k_norm2_max) (Cauchy-Schwarz: always valid) and the call enqueues a PAIR of launches over the same
 *   grid: units whose bound is <= 56 run the FAST body with that bound as softmax reference, the others the general body; the
 *   workgroups of the other kind exit at once.  No host round trip, no global state, hipGraph-capturable.  Cost over a host-promised
 *   FAST call: the norm pass (HBM-bound) + one launch of early-exiting workgroups. */
int osk_rownorm2_max_bf16(const void* x, int64_t batch_stride, int64_t row_stride, int B, int L, int H, int hd,
                          float* out, int accumulate, void* stream);
int osk_attention_fwd_auto_bf16(const void* q, int64_t q_batch_stride, int64_t q_row_stride,
                           const void* k, int64_t k_seg_stride, int64_t k_batch_stride, int64_t k_row_stride,
                           const void* vt, int64_t vt_seg_stride,
                           void* out, int64_t o_batch_stride, int64_t o_row_stride,
                           float* lse, int B, int H, int Lq, int n_seg, int seg_len, int hd,
                           float scale, int q_prescaled, int kv_batches, const float* q_norm2_max, const float* k_norm2_max,
                           void* workspace, int64_t workspace_bytes, void* stream);

/* ---- merge of S attention results over DISJOINT key sets by their log-sum-exp.
 * replaces _rescale_out_lse / the per-hop update of the ring attention (opensora/models/mmdit/distributed.py:223-313), applied
 * once to all S parts: the sequence-parallel K / V^T all-gather cut into S key slices (open_sora_amd/seqpar.py, kv_chunks) runs
 * osk_attention_fwd_bounded_bf16 on slice s as soon as gather s has arrived and combines the S (out, lse) pairs here.
 * parts   bf16 [S, B, L, H*hd]: row (s, b, l) at parts + s*part_stride + b*p_batch_stride + l*p_row_stride (elements, multiples
 *         of 8; row strides >= H*hd; 16-byte aligned pointer; last dim contiguous)
 * lse     f32 [S, B, H, L] contiguous, natural log, as osk_attention_fwd_bf16 writes it; -inf = a part that saw no key
 * out     bf16 [B, L, H*hd] with its own batch / row strides (same rules); must not overlap parts
 * lse_out f32 [B, H, L] contiguous, or NULL
 * Per (b, l, h):  m = max_s lse_s,  w_s = exp(lse_s - m) (0 for lse_s = -inf),  out = bf16(sum_s w_s part_s / sum_s w_s) with the
 * sums in f32 and ONE rounding,  lse_out = m + log sum_s w_s.  Every lse_s = -inf: out = 0 and lse_out = -inf, never NaN.
 * 1 <= S <= 8 and hd % 8 == 0 (else OSK_EINVAL); H <= 512 and B <= 65535 (else OSK_EUNSUPPORTED).  HBM-bound: (S + 1) row images,
 * 16-byte loads and stores, each lse value read once per (row, head).  No allocation, no memset, no synchronisation: capturable
 * in a hipGraph. */
int osk_attention_merge_bf16(const void* parts, int64_t part_stride, int64_t p_batch_stride, int64_t p_row_stride,
                             const float* lse, void* out, int64_t o_batch_stride, int64_t o_row_stride, float* lse_out,
                             int S, int B, int H, int L, int hd, void* stream);

/* ---- fp8 P.V variant of the attention (opt-in fp8 mode, BASELINE configs[4]; head_dim 72 / 128): QK^T, the softmax and
 * the output as osk_attention_fwd_ws_bf16, but P (<= 2^8 by construction) and V^T are OCP e4m3 and a 64-key tile's P.V
 * is one v_mfma_f32_32x32x64_f8f6f4 per O^T row tile.
 * osk_v_transpose_fp8: V bf16 [B, L, H*hd] view -> vt8 e4m3 bytes [B, H, RP, Lp], RP = (hd + 1) rounded up to 16
 *   (80 / 144), Lp = L rounded up to 64: rows 0..hd-1 = clamp(V / scales[b*H + h]) in the key order the kernel's
 *   accumulator layout dictates, row hd = 1.0 for keys < L else 0 (softmax denominator / key validity), further rows 0.
 *   scales f32 [B, H] (device memory; typically absmax over the head / 448, computed by the caller).
 * osk_attention_fwd_pv8_bf16: vt8 from the call above (per key segment, vt8_seg_stride in BYTES), v_scale = the same
 *   scales indexed by (key batch, head); everything else as osk_attention_fwd_ws_bf16. */
/* osk_v_scale_fp8: scales[b*H + h] = absmax(V[b, :, h, :]) / 448 (1.0 for an all-zero head): the e4m3 scales
 * osk_v_transpose_fp8 / osk_attention_fwd_pv8_bf16 take.  (Under sequence parallelism max-reduce them over the ranks.) */
int osk_v_scale_fp8(const void* v, int64_t v_batch_stride, int64_t v_row_stride, float* scales, int B, int L, int H,
                    int hd, void* stream);
/* osk_kv_scale_fp8: the scales of K and of V from ONE launch, into one contiguous buffer scales f32 [2, B, H]:
 *   scales[0][b][h] = what osk_v_scale_fp8 returns when it is pointed at K, scales[1][b][h] = what it returns for V, bit for bit
 *   (absmax / 448, the division in IEEE f32, 1.0 for an all-zero head).  k, v: bf16 [B, L, H*hd] views with their own batch and
 *   row strides (elements, multiples of 8; 16-byte aligned pointers; last dim contiguous); hd a multiple of 8 (<= 8192), H <= 256.
 *   For the qk8 attention under sequence parallelism: both vectors must be the same on every rank, and one buffer means ONE
 *   max-reducing collective per block (open_sora_amd/seqpar.py), after which osk_k_pack_fp8 and osk_v_transpose_fp8 take the two
 *   halves.  One workgroup per (tensor, batch, head) walks all L rows of its head with the loads of a round in flight before the
 *   first use: a workgroup's maximum is final when it ends, which is what lets one launch do without a zeroed accumulator.  The
 *   price: 2 * B * H workgroups is all the parallelism there is -- HBM-bound from about 150 of them, below that bound by the
 *   CUs in use (48 workgroups of a rank of the 11B model: 2.0 TB/s, 0.17 ms for 355 MB; profiles/attn_qk8_sp.md).  No
 *   allocation, no memset, no atomics on global memory, no synchronisation: capturable in a hipGraph. */
int osk_kv_scale_fp8(const void* k, int64_t k_batch_stride, int64_t k_row_stride,
                     const void* v, int64_t v_batch_stride, int64_t v_row_stride, float* scales,
                     int B, int L, int H, int hd, void* stream);
int osk_v_transpose_fp8(const void* v, int64_t v_batch_stride, int64_t v_row_stride, const float* scales, void* vt8,
                        int B, int L, int H, int hd, void* stream);
int osk_attention_fwd_pv8_bf16(const void* q, int64_t q_batch_stride, int64_t q_row_stride,
                               const void* k, int64_t k_seg_stride, int64_t k_batch_stride, int64_t k_row_stride,
                               const void* vt8, int64_t vt8_seg_stride, const float* v_scale,
                               void* out, int64_t o_batch_stride, int64_t o_row_stride,
                               float* lse, int B, int H, int Lq, int n_seg, int seg_len, int hd,
                               float scale, int q_prescaled, int kv_batches, void* workspace, int64_t workspace_bytes,
                               void* stream);

/* ---- fp8 QK^T + fp8 P.V variant of the attention (opt-in fp8 mode, qk8; head_dim 128 only, other head dims: OSK_EUNSUPPORTED).
 * Reference call site: attention() of opensora/models/mmdit/math.py:16-36, like the entries above.  Both products of a 64-key
 * tile run on v_mfma_f32_32x32x64_f8f6f4; P.V, V^T (osk_v_transpose_fp8), the softmax bookkeeping and the output are those of
 * osk_attention_fwd_pv8_bf16.
 * osk_k_pack_fp8: K bf16 [B, L, H*128] view (the output of osk_qknorm_rope_bf16, strides in elements, last dim contiguous) ->
 *   k8 e4m3 bytes [B, H, Lp, 128], Lp = L rounded up to 64.  Quantisation rule: byte d of row l of head (b, h) =
 *   e4m3(clamp(K[b, l, h, d] / scales[b*H + h], -448, 448)), the division in f32 (IEEE), the conversion round-to-nearest-even,
 *   saturating.  Byte order: natural -- dim d is byte d of its row; the kernel's LDS image is a straight LDS-DMA copy of 16-byte
 *   pieces of these rows (the bank swizzle is in the copy's addresses, not in the tensor).  Rows L .. Lp-1 repeat row L-1, so
 *   the scores of a ragged last tile stay finite; key validity comes from the baked row of vt8.  scales f32 [B, H]: what
 *   osk_v_scale_fp8 computes when it is pointed at K (absmax over the head / 448, 1.0 for an all-zero head).  With several key
 *   segments: one call per segment with the SAME scales (their maximum over the segments).  Sequence parallelism uses exactly
 *   that: every rank packs its own segment with the max-reduced scales of osk_kv_scale_fp8, the packed segments are all-gathered
 *   (K travels at 1 byte per element), and the gathered bytes are the ones one device packs from the whole K (padding rows of a
 *   ragged segment aside).
 * osk_attention_fwd_qk8_bf16: the arguments of osk_attention_fwd_pv8_bf16 except that k8 (from the call above, per key segment)
 *   replaces k with k8_seg_stride and k8_batch_stride in BYTES (multiples of 16; batch stride of one segment's tensor =
 *   H * Lp * 128), k8_row_stride = 128 (bytes; anything else: OSK_EUNSUPPORTED), and k_scale = the scales the pack used, indexed
 *   by (key batch, head).  Q stays bf16 in memory; the kernel quantises it in its prologue, per query row and head:
 *   qf = f32(q) * (q_prescaled ? 1 : scale * log2(e)), s_q = absmax over the head's 128 dims of qf / 448 (1.0 for an all-zero
 *   row), q8 = e4m3(clamp(qf / s_q, -448, 448)), same rounding.  A score in log2 units is s_q * k_scale * (q8 . k8), applied
 *   with one f32 FMA per score.  No allocation, no synchronisation, no memset: capturable in a hipGraph. */
int osk_k_pack_fp8(const void* k, int64_t k_batch_stride, int64_t k_row_stride, const float* scales, void* k8,
                   int B, int L, int H, int hd, void* stream);
int osk_attention_fwd_qk8_bf16(const void* q, int64_t q_batch_stride, int64_t q_row_stride,
                               const void* k8, int64_t k8_seg_stride, int64_t k8_batch_stride, int64_t k8_row_stride,
                               const float* k_scale, const void* vt8, int64_t vt8_seg_stride, const float* v_scale,
                               void* out, int64_t o_batch_stride, int64_t o_row_stride,
                               float* lse, int B, int H, int Lq, int n_seg, int seg_len, int hd,
                               float scale, int q_prescaled, int kv_batches, void* workspace, int64_t workspace_bytes,
                               void* stream);

/* ---- attention over key segments whose LAST one is shorter (sequence parallelism over a token count L the rank count P does not
 * divide: ranks 0 .. P-2 own Lc = ceil(L / P) rows, the last one Lt = L - (P-1) Lc; open_sora_amd/seqpar.py).  The reference refuses
 * such lengths (opensora/models/mmdit/distributed.py:604-608); the arithmetic replaced is that of the entries above.
 * The hand-scheduled kernels bake one ragged-tile mask per launch, so the call enqueues, on `stream`:
 *   A  the n_seg - 1 full segments (seg_len keys each) into out / lse, exactly as the entry of that operand kind would,
 *   B  the last segment alone (n_seg = 1, seg_len = last_seg_len, down to one key) into f32 partials in the workspace,
 *   M  one in-place merge of B's partial into A's rows by their log-sum-exp (osk_attention_merge_into_bf16's kernel).
 * Each launch picks its loop body by the normal rules (A with several segments of fewer than 3 tiles: the general body).
 * mode: which operands k / vt are, shared by both launches --
 *   OSK_ATTN_BF16  as osk_attention_fwd_bounded_bf16 (score_bound as there; k_scale, v_scale ignored),
 *   OSK_ATTN_PV8   as osk_attention_fwd_pv8_bf16   (vt = vt8, vt_seg_stride in bytes, v_scale; score_bound must be 0 or is ignored),
 *   OSK_ATTN_QK8   as osk_attention_fwd_qk8_bf16   (k = k8 with byte strides, k_row_stride = 128, k_scale; vt = vt8, v_scale).
 * Layout of the last segment: n_seg - 1 segment strides behind the first, written as a tensor of last_seg_len keys OF ITS OWN -- V^T
 *   rows of round_up(last_seg_len, 64) positions (what osk_v_transpose_bf16 / osk_v_transpose_fp8 write for L = last_seg_len), e4m3 K
 *   [Bkv, H, round_up(last_seg_len, 64), 128] (osk_k_pack_fp8 for L = last_seg_len); bf16 K keeps k_batch_stride / k_row_stride.
 * out: 16-byte aligned, strides multiples of 8 (the merge moves 16-byte pieces); lse f32 [B, H, Lq] or NULL.
 * workspace: required (NULL or fewer bytes than the partials need: OSK_EINVAL); osk_attention_ragged_workspace_bytes(B, H, Lq, hd) is
 *   always enough and leaves launch A the tail-split room of osk_attention_workspace_bytes().
 * 2 <= n_seg, 1 <= last_seg_len <= seg_len (else OSK_EINVAL).  No allocation, no memset, no host synchronisation: capturable in a
 * hipGraph.  Cost over one launch on a divisible length: one more launch (its workgroups walk one segment) + the merge, which
 * moves 8 bytes per output element. */
#define OSK_ATTN_BF16 0
#define OSK_ATTN_PV8 1
#define OSK_ATTN_QK8 2
int64_t osk_attention_ragged_workspace_bytes(int B, int H, int Lq, int hd);
int osk_attention_fwd_ragged_bf16(const void* q, int64_t q_batch_stride, int64_t q_row_stride,
                                  const void* k, int64_t k_seg_stride, int64_t k_batch_stride, int64_t k_row_stride,
                                  const float* k_scale, const void* vt, int64_t vt_seg_stride, const float* v_scale,
                                  void* out, int64_t o_batch_stride, int64_t o_row_stride, float* lse,
                                  int B, int H, int Lq, int n_seg, int seg_len, int last_seg_len, int hd,
                                  float scale, int q_prescaled, int kv_batches, float score_bound, int mode,
                                  void* workspace, int64_t workspace_bytes, void* stream);
/* The merge on its own: fold the result of a second attention over OTHER keys into a finished (out, lse) pair, in place.
 * out   bf16 [B, Lq, H*hd] view (16-byte aligned, strides multiples of 8, row stride >= H*hd): read and overwritten
 * lse   f32 [B, H, Lq] contiguous, natural log: read and overwritten with the merged value
 * o_b   f32 [B, H, Lqp, hd] contiguous, Lqp = Lq rounded up to 256 (rows >= Lq are never read), 16-byte aligned: normalised partial
 * lse_b f32 [B, H, Lqp] contiguous, natural log; -inf = a part that saw no key (its o_b row is then not used)
 * Per (b, l, h) as osk_attention_merge_bf16 with S = 2: f32 sums, ONE rounding; both -inf: out = 0, lse = -inf.
 * hd in {64, 72, 128} (else OSK_EUNSUPPORTED).  HBM: out read + written (2 + 2 bytes per element) + o_b read (4): no third image
 * of the rows, where osk_attention_merge_bf16 with S = 2 moves 6 bytes per element and needs two partial images beside out. */
int osk_attention_merge_into_bf16(void* out, int64_t o_batch_stride, int64_t o_row_stride, float* lse, const float* o_b,
                                  const float* lse_b, int B, int H, int Lq, int hd, void* stream);
/* The same with TWO partials (o_b, lse_b) and (o_c, lse_c), each laid out as above, folded into (out, lse) in ONE pass (an additive
 * entry, the version stays 2): per (b, l, h) osk_attention_merge_bf16 with S = 3 -- f32 sums, ONE rounding.  A part whose lse is
 * -inf contributes nothing (its row may hold anything); all three -inf: out = 0, lse = -inf, never NaN.  Arguments, alignment and
 * status codes as osk_attention_merge_into_bf16 (o_c, lse_c as o_b, lse_b); hd in {64, 72, 128}.  HBM per output element: out read
 * + written (2 + 2) + two f32 partials (4 + 4) = 12 bytes in 16-byte loads and stores, where two passes of the entry above move
 * 16 and round twice.  No allocation, no memset, no atomics, no synchronisation: capturable in a hipGraph. */
int osk_attention_merge_into2_bf16(void* out, int64_t o_batch_stride, int64_t o_row_stride, float* lse, const float* o_b,
                                   const float* lse_b, const float* o_c, const float* lse_c, int B, int H, int Lq, int hd,
                                   void* stream);

/* ---- frame-window attention: every 256-row query block sees an always-attended key prefix and ONE run of 64-key tiles of the rest
 * (opt-in; an additive entry, the version stays 2).  It replaces nothing in the reference: opensora/models/mmdit/math.py:22-36 lets
 * every query see every key.  It is what a video DiT's sliding-window option computes when text stays global and an image query
 * keeps the frames around its own, stated as a mask and exact with respect to that mask:
 *   keys [0, n_prefix)   the prefix (text): seen by every query.  n_prefix % 64 == 0, 0 <= n_prefix < Lk
 *   keys [n_prefix, Lk)  the body; table tile j = body keys 64 j .. 64 j + 63 (the last tile may be ragged)
 *   windows              DEVICE int32 [n_windows][2] = (first tile, tile count) per 256-row query block, n_windows = ceil(Lq / 256):
 *                        rows 256 i .. 256 i + 255 see the prefix and body tiles [first, first + count) and NOTHING else.
 *                        The kernel clamps a row to 0 <= first < tiles, 1 <= count <= tiles - first: a bad table gives wrong
 *                        numbers, never an out-of-range address (open_sora_amd/_C.py validates the host copy and raises).
 * q, k, out, lse, scale, q_prescaled, kv_batches, score_bound: as osk_attention_fwd_bounded_bf16 with ONE key segment of Lk keys
 * (k bf16 [Bkv, Lk, H*hd] view; vt = osk_v_transpose_bf16 of all Lk keys, [Bkv, H, hd, round_up(Lk, 64)]); the bound covers prefix
 * and body alike and selects the FAST body of both launches (0: the general body).  The call enqueues, on `stream`:
 *   A  the body as a key axis of its own (K, V^T advanced by n_prefix keys) with the table, finished rows into out / lse,
 *   B  the prefix alone into f32 partials in the workspace (every work unit, one part),
 *   M  one in-place merge of B's partial into A's rows by their log-sum-exp (osk_attention_merge_into_bf16's kernel).
 * n_prefix == 0: launch A alone, workspace may be NULL; with full windows the result is bit-identical to osk_attention_fwd_bf16.
 * n_prefix > 0: out 16-byte aligned with strides multiples of 8, workspace required -- osk_attention_window_workspace_bytes(B, H,
 * Lq, hd) is always enough (f32 partials + launch A's lse when the caller keeps none).
 * OSK_EINVAL: n_windows != ceil(Lq / 256), NULL / misaligned table, n_prefix not a multiple of 64 or >= Lk, missing / short
 * workspace with n_prefix > 0, negative or NaN score_bound.  hd in {64, 72, 128} (else OSK_EUNSUPPORTED).  bf16 operands; the fp8
 * operand kinds have the entry below.
 * No allocation, no memset, no host synchronisation: capturable in a hipGraph.
 * Cost: work units are always 256 rows (no wide head_dim-72 layout) and the grid's last round is not split along the keys; a
 * unit's time follows its tile count, so the launch ends with its longest windows.  On top of launch A: launch B walks n_prefix
 * keys per unit and the merge moves 8 bytes per output element.  Measured: profiles/attn_window.md. */
int64_t osk_attention_window_workspace_bytes(int B, int H, int Lq, int hd);
int osk_attention_fwd_window_bf16(const void* q, int64_t q_batch_stride, int64_t q_row_stride,
                                  const void* k, int64_t k_batch_stride, int64_t k_row_stride, const void* vt,
                                  void* out, int64_t o_batch_stride, int64_t o_row_stride, float* lse,
                                  int B, int H, int Lq, int Lk, int n_prefix, int hd, float scale, int q_prescaled,
                                  int kv_batches, float score_bound, const int32_t* windows, int n_windows,
                                  void* workspace, int64_t workspace_bytes, void* stream);
/* The same entry in fp8 mode (an additive entry, the version stays 2).  Like the entry above it replaces nothing in the reference
 * -- opensora/models/mmdit/math.py:22-36 lets every query see every key -- and the arithmetic under the mask is that of
 * osk_attention_fwd_pv8_bf16 / osk_attention_fwd_qk8_bf16.  Mask, exactly as above: keys [0, n_prefix) are seen by every query; rows
 * 256 i .. 256 i + 255 see, of the body keys [n_prefix, Lk), the 64-key tiles [first, first + count) of windows[i] and NOTHING
 * else; the kernel clamps a table row as above.  Arguments: those of osk_attention_fwd_window_bf16 without score_bound (the fp8
 * kernels have no bounded body), plus the scales and
 *   mode  OSK_ATTN_PV8  hd in {72, 128}: k = the bf16 K [Bkv, Lk, H*hd] view, read in place (strides in elements);
 *                       vt = the e4m3 V^T of ALL Lk keys from osk_v_transpose_fp8, [Bkv, H, RP, Lp], Lp = round_up(Lk, 64);
 *                       v_scale f32 [Bkv, H]; k_scale ignored.
 *         OSK_ATTN_QK8  hd == 128 only: k = the e4m3 K of all Lk keys from osk_k_pack_fp8, [Bkv, H, Lp, 128], k_batch_stride in BYTES
 *                       (a non-negative multiple of 16), k_row_stride = 128 (anything else: OSK_EUNSUPPORTED); k_scale f32 [Bkv, H]
 *                       = the scales the pack used; vt, v_scale as for OSK_ATTN_PV8.  Q stays bf16 and is quantised in the kernel
 *                       prologue per query row and head, as osk_attention_fwd_qk8_bf16 states.
 *         OSK_ATTN_BF16 OSK_EINVAL (that is the entry above).
 * The call enqueues the launches A, B, M of the entry above on the pv8 / qk8 kernels: A enters K and V^T n_prefix keys in (n_prefix
 * rows of K; n_prefix bytes along the key axis of every V^T row, the validity row included) and keeps the head and batch strides of
 * the whole tensors; B walks the prefix from the tensors' origin with the same scales.
 * n_prefix == 0: launch A alone, workspace may be NULL; with full windows the result is bit-identical to osk_attention_fwd_pv8_bf16
 * / osk_attention_fwd_qk8_bf16 called without a workspace.  n_prefix > 0: out 16-byte aligned with strides multiples of 8,
 * workspace required -- osk_attention_window_workspace_bytes(B, H, Lq, hd) is always enough.  lse: f32 [B, H, Lq] or NULL.
 * OSK_EINVAL: the list of the entry above, NULL or misaligned scales (v_scale; k_scale in qk8 mode), a k_batch_stride that is no
 * non-negative multiple of 16 in qk8 mode, a mode other than the two.  OSK_EUNSUPPORTED: hd outside the mode's set, k_row_stride
 * != 128 in qk8 mode.  A refused call launches nothing.  No allocation, no memset, no host synchronisation: capturable in a hipGraph.
 * Cost: as above; the V^T pack (and in qk8 mode the K pack) in front of the call still touch every key.  profiles/attn_window.md. */
int osk_attention_fwd_window_fp8_bf16(const void* q, int64_t q_batch_stride, int64_t q_row_stride,
                                      const void* k, int64_t k_batch_stride, int64_t k_row_stride, const float* k_scale,
                                      const void* vt, const float* v_scale, void* out, int64_t o_batch_stride,
                                      int64_t o_row_stride, float* lse, int B, int H, int Lq, int Lk, int n_prefix, int hd,
                                      float scale, int q_prescaled, int kv_batches, int mode, const int32_t* windows,
                                      int n_windows, void* workspace, int64_t workspace_bytes, void* stream);
/* The window entries with always-attended TRAILING keys as well (an additive entry, the version stays 2): the mask a windowed video
 * DiT wants for its conditioning ("anchor" / "sink") frames -- leading frames extend the prefix behind the text, trailing frames are
 * the suffix.  Like the entries above it replaces nothing in the reference.  Mask, exact:
 *   keys [0, n_prefix)    seen by every query.  n_prefix % 64 == 0, 0 <= n_prefix
 *   keys [s0, Lk)         s0 = Lk - n_suffix: seen by every query.  n_suffix >= 0; with n_suffix > 0, s0 % 64 == 0 and s0 > n_prefix
 *                         (the body keeps at least one tile); the tensor's last tile may be ragged (the kernels' own tail mask)
 *   keys [n_prefix, s0)   the body; table tile j = body keys 64 j .. 64 j + 63 -- with n_suffix > 0 all whole tiles;
 *                         rows 256 i .. 256 i + 255 see the tiles [first, first + count) of windows[i] and NOTHING else of the body.
 *                         The kernel clamps a row to 0 <= first < tiles, 1 <= count <= tiles - first (a count of 0 is NOT an empty
 *                         run: it reads as 1).
 * Arguments: those of osk_attention_fwd_window_bf16 / osk_attention_fwd_window_fp8_bf16 (k_scale, v_scale: ignored by the modes
 * that have none; score_bound: OSK_ATTN_BF16 only, ignored otherwise) plus n_suffix, and mode = OSK_ATTN_BF16 | OSK_ATTN_PV8 |
 * OSK_ATTN_QK8 with the operands of osk_attention_fwd_ragged_bf16 for ONE key segment of Lk keys.  The call enqueues, on `stream`:
 *   A  the body [n_prefix, s0) as a key axis of its own with the table, finished rows into out / lse,
 *   B  the prefix from the tensors' origin into f32 partials in the workspace (every work unit, one part),
 *   C  the suffix, entered s0 keys in as A is entered n_prefix keys in, into a second set of f32 partials,
 *   M  ONE in-place three-part merge of B and C into A's rows (osk_attention_merge_into2_bf16's kernel: one rounding).
 * n_suffix == 0: the launches and the result of the window entry of that mode, bit for bit.  n_prefix == 0 < n_suffix: A, C and
 * the two-part merge.  Workspace: osk_attention_window_anchor_workspace_bytes(B, H, Lq, hd) (two partial sets + launch A's lse when
 * the caller keeps none) is always enough; out 16-byte aligned, strides multiples of 8.
 * OSK_EINVAL: the lists of the two entries above; a negative n_suffix, Lk - n_suffix no multiple of 64 or <= n_prefix (a suffix that
 * reaches the prefix), a workspace short of what the launches in use need, a mode other than the three.  OSK_EUNSUPPORTED: as
 * there.  A refused call launches nothing.  No allocation, no memset, no host synchronisation: capturable in a hipGraph.
 * Cost over the window entry: launch C walks n_suffix keys per unit, B the longer prefix, and the merge moves 12 bytes per output
 * element instead of 8.  Measured: profiles/attn_window.md. */
int64_t osk_attention_window_anchor_workspace_bytes(int B, int H, int Lq, int hd);
int osk_attention_fwd_window_anchor_bf16(const void* q, int64_t q_batch_stride, int64_t q_row_stride,
                                         const void* k, int64_t k_batch_stride, int64_t k_row_stride, const float* k_scale,
                                         const void* vt, const float* v_scale, void* out, int64_t o_batch_stride,
                                         int64_t o_row_stride, float* lse, int B, int H, int Lq, int Lk, int n_prefix,
                                         int n_suffix, int hd, float scale, int q_prescaled, int kv_batches, float score_bound,
                                         int mode, const int32_t* windows, int n_windows, void* workspace,
                                         int64_t workspace_bytes, void* stream);

/* ---- short-sequence attention with an optional ALiBi bias (the STDiT-generation block's temporal
 * self-attention over T <= 64 frames, B * H * W independent sequences, "RoPE/ALiBi" in BASELINE.json's north_star).  The mounted
 * v2.0 reference passes alibi_slopes=None at every flash-attn call site (opensora/models/mmdit/math.py:22-36), so this entry is
 * PARITY-UNPINNED; semantics = flash-attn's documented `alibi_slopes`:
 *   out[b, i, h] = softmax_j(scale * q_i . k_j - alibi_slopes[h] * |i + Lk - Lq - j|) v_j ,   Lq, Lk <= 64
 * q, k, v, out bf16 [B, L, H * hd] views (row strides in elements, last dim contiguous), alibi_slopes f32 [H] or NULL (no bias).
 * One wave per (batch, head), registers only, HBM-bound; V is taken as is (no osk_v_transpose_bf16).  hd in {64, 72, 128};
 * longer sequences: OSK_EUNSUPPORTED (use osk_attention_fwd_bf16). */
int osk_attention_short_bf16(const void* q, int64_t q_batch_stride, int64_t q_row_stride, const void* k, int64_t k_batch_stride,
                             int64_t k_row_stride, const void* v, int64_t v_batch_stride, int64_t v_row_stride, void* out,
                             int64_t o_batch_stride, int64_t o_row_stride, const float* alibi_slopes, int B, int H, int Lq, int Lk,
                             int hd, float scale, void* stream);

/* ---- self-attention with a learned relative-position bias: the attention of the T5 text encoder.
 * replaces T5Attention.forward inside the Hugging Face T5EncoderModel that HFEmbedder runs (opensora/models/text/conditioner.py:48-53:
 * T5-v1.1-XXL, 512 tokens, attention_mask=None -- pad tokens are attended).  T5 self-attention is non-causal, does not scale its
 * scores (the caller passes scale = 1.0) and adds a per-head bias that depends on the relative distance j - i alone:
 *   out[b, i, h] = sum_j softmax_j(scale * q_i . k_j + bias[h * bias_row_stride + (j - i) + (L - 1)]) v_j ,   Lq = Lk = L
 * q, k, v, out bf16 [B, L, H * hd] views (batch / row strides in elements, last dim contiguous: q, k, v may be the three column
 * groups of one fused [B, L, 3 * H * hd] projection output); V is taken as is (no osk_v_transpose_bf16).  bias f32
 * [H, >= 2 L - 1] indexed by distance (open_sora_amd/t5.py expands T5's 32-bucket embedding into it once per L), or NULL (no
 * bias).  Scores, bias add and online softmax in f32; no L x L matrix in memory.  hd == 64 and 1 <= L <= 4096, any L (key tails
 * are masked, query rows >= L never stored); another hd or a longer L: OSK_EUNSUPPORTED. */
int osk_attention_relbias_bf16(const void* q, int64_t q_batch_stride, int64_t q_row_stride, const void* k, int64_t k_batch_stride,
                               int64_t k_row_stride, const void* v, int64_t v_batch_stride, int64_t v_row_stride, void* out,
                               int64_t o_batch_stride, int64_t o_row_stride, const float* bias, int64_t bias_row_stride, int B,
                               int H, int L, int hd, float scale, void* stream);

/* name of the device kernel osk_attention_fwd_bf16 dispatches to for (hd, seg_len) (reporting only: bench.py labels its
 * roofline line and the rocprof stats with it). */
const char* osk_attention_kernel_name(int hd, int seg_len);
/* ... and of the loop BODY a call of osk_attention_fwd_bounded_bf16 with this segment layout and score bound runs (reporting /
 * tests only): "attn_asm72_kernel<FAST>" = the bounded body (no max tracking; needs 0 < score_bound <= 56 and, with several key
 * segments, segments of >= 3 tiles), "attn_asm72_kernel<general>" = the running-reference body (head_dim 64 runs the head_dim-72 kernels).  The
 * choice is data-dependent through score_bound (open_sora_amd/mmdit.py derives it from the QK-norm scale vectors of
 * opensora/models/mmdit/layers.py:113-135), so bench.py prints it next to the timing. */
const char* osk_attention_body_name(int hd, int n_seg, int seg_len, float score_bound);

/* ---- classifier-free-guidance combine + Euler step of the rectified-flow sampler (f32 math):
 *   v = u2 + g_img*(u - u2) + g_txt*(c - u);  x_out = x + dt * v
 * replaces opensora/utils/sampling.py:217-222.  pred bf16 [3, n] = (cond, uncond, uncond_2) chunks,
 * x bf16 [n], x_out bf16 [n].  g_img_vec (f32 [n]) overrides the scalar g_img when non-NULL
 * (temporal guidance ramp, sampling.py:209-216). */
int osk_cfg_euler_bf16(const void* pred, int64_t n, const void* x, void* x_out,
                       float g_txt, float g_img, const float* g_img_vec, float dt, void* stream);

/* ---- the same combine + Euler step over the nb leading branches of the triple, for sampler steps that did not run the
 * branches their guidance cancels (replaces opensora/utils/sampling.py:208-222, which always combines three):
 *   nb 3:  v = u2 + g_img*(u - u2) + g_txt*(c - u)     the arithmetic of osk_cfg_euler_bf16, same operation order, same bits
 *   nb 2:  v = u + g_txt*(c - u)                        branches 2 and 3 identical (u2 == u); g_img, g_img_vec ignored
 *   nb 1:  v = c                                        both guidances 1.0; g_txt, g_img, g_img_vec ignored
 *   x_out = x + dt * v                                  f32 math, one rounding; x_out == x (in place) is allowed
 * pred bf16 [nb, n]: exactly nb * n elements are read.  Another nb, a NULL pred / x / x_out or n % 8 != 0: OSK_EINVAL, no launch. */
int osk_cfg_euler_nb_bf16(const void* pred, int nb, int64_t n, const void* x, void* x_out,
                          float g_txt, float g_img, const float* g_img_vec, float dt, void* stream);

/* ---- strided row copy: dst[j, b, l, 0:C] = src[j, b, l, 0:C] (bf16; element strides; src_batch_stride 0 broadcasts one item).
 * replaces the host-side tensor glue of a denoise step: `torch.cat([img, img, img])` of the CFG triple
 * (opensora/utils/sampling.py:196-201), the operand assembly in front of img_in / cond_in (opensora/models/mmdit/model.py:170-176),
 * and -- with n_chunks = P -- the two rearranges around the head all-to-all of the sequence-parallel attention
 * (opensora/models/mmdit/distributed.py:473-495: [B, L/P, P x Dg] <-> [P, B, L/P, Dg]; the token-major side has chunk stride Dg).
 * C and all strides multiples of 4 elements, pointers 8-byte aligned. */
int osk_copy_rows_bf16(const void* src, int64_t src_chunk_stride, int64_t src_batch_stride, int64_t src_row_stride, void* dst,
                       int64_t dst_chunk_stride, int64_t dst_batch_stride, int64_t dst_row_stride, int n_chunks, int B, int L, int C,
                       void* stream);

/* ---- step cache of the sampler (not in the reference; open_sora_amd/sampling.py, I2VDenoiser.denoise(step_cache=...)).  Additive
 * under ABI version 2.
 * Step delta, one pass over two bf16 [B, L, C] tensors:
 *   sums[0] = sum |cur - prev|,  sums[1] = sum |prev|   (f32 accumulation),  then prev := cur, bit for bit.
 * cur: a view with element strides cur_batch_stride / cur_row_stride (multiples of 8, unit channel stride); prev: contiguous, must
 * not overlap cur.  Two stages and no atomics: per-workgroup f32 partials go to `workspace`
 * (osk_step_delta_workspace_bytes(B, L, C) bytes, 4-byte aligned), a one-workgroup finish adds them in a fixed order -- the same
 * inputs give the same bits on every call.  The host forms the ratio (one 8-byte read back).  C % 8 == 0, cur / prev 16-byte aligned,
 * B L C / 8 < 2^31; anything else (a NULL pointer, a workspace too small) is OSK_EINVAL with nothing launched.  No allocation,
 * memset or synchronisation: capturable. */
int64_t osk_step_delta_workspace_bytes(int B, int L, int C);
int osk_step_delta_bf16(const void* cur, int64_t cur_batch_stride, int64_t cur_row_stride, void* prev, float* sums, int B, int L, int C,
                        void* workspace, int64_t workspace_bytes, void* stream);

/* The step cache under sequence parallelism (open_sora_amd/mmdit.py, MMDiTModel.step_head on a sharded model).  Additive under ABI
 * version 2.  Every rank's osk_step_delta_bf16 gives the pair of its own rows; after one all-gather every rank holds
 * pairs f32 [P, 2] (slot r: rank r's (sum |cur - prev|, sum |prev|)).  This entry adds them in rank order 0 .. P-1 with plain f32
 * adds on one lane:  sums[j] = ((pairs[0][j] + pairs[1][j]) + ...) + pairs[P-1][j], at most P - 1 roundings; NaN and infinity
 * propagate.  Equal gathered bits give equal sums on every rank, which is the whole synchronisation of the decision.  pairs and sums
 * 4-byte aligned, P >= 1; a NULL pointer, P < 1 or a misaligned pointer is OSK_EINVAL with nothing launched.  sums must not
 * overlap pairs.  No allocation, memset or synchronisation: capturable. */
int osk_step_sums_combine_f32(const float* pairs, int P, float* sums, void* stream);

/* Residual store and apply over strided bf16 [B, L, C] views (strides multiples of 8, unit channel stride, 16-byte aligned,
 * C % 8 == 0):  out = bf16(f32(a) - f32(b))  /  out = bf16(f32(a) + f32(b)), the exact difference / sum rounded once.  out may be a
 * or b (same strides) -- the sampler stores R = Y - X over the X it saved, and applies Y = X + R over X. */
int osk_residual_sub_bf16(const void* a, int64_t a_batch_stride, int64_t a_row_stride, const void* b, int64_t b_batch_stride,
                          int64_t b_row_stride, void* out, int64_t out_batch_stride, int64_t out_row_stride, int B, int L, int C,
                          void* stream);
int osk_residual_add_bf16(const void* a, int64_t a_batch_stride, int64_t a_row_stride, const void* b, int64_t b_batch_stride,
                          int64_t b_row_stride, void* out, int64_t out_batch_stride, int64_t out_row_stride, int B, int L, int C,
                          void* stream);

/* ---- attention broadcast of the sampler (not in the reference; open_sora_amd/sampling.py, I2VDenoiser.denoise(attn_broadcast=...)).
 * Additive under ABI version 2.  The store and the load of one block's attention output: a copy of bf16 [B, L, C] between two
 * strided views (element strides, multiples of 8; unit channel stride; 16-byte aligned; C % 8 == 0; B L C / 8 < 2^31), one of which
 * is a cache slot of `cache_rows` batch rows:
 *   to_cache != 0 (store):  dst[row_map[b], l, 0:C] = src[b, l, 0:C]         dst is the slot
 *   to_cache == 0 (load):   dst[b, l, 0:C]          = src[row_map[b], l, 0:C]  src is the slot
 * row_map: int32 [B] on the DEVICE (a captured graph replays it), distinct entries, or NULL for the identity (then B <= cache_rows).
 * A batch item whose map entry lies outside [0, cache_rows) is skipped, nothing read or written.  The two views must not overlap.
 * Anything else (a NULL view, a stride that lets batch items overlap, ...) is OSK_EINVAL with nothing launched.  No allocation,
 * memset or synchronisation: capturable. */
int osk_attn_cache_copy_bf16(const void* src, int64_t src_batch_stride, int64_t src_row_stride, void* dst, int64_t dst_batch_stride,
                             int64_t dst_row_stride, const int32_t* row_map, int cache_rows, int to_cache, int B, int L, int C,
                             void* stream);

/* =====================================================================================================
 * Causal 3-D VAE (HunyuanVideo VAE, /root/reference/opensora/models/hunyuan_vae).  Activations are channels-last
 * NDHWC bf16 ([B, T, H, W, C] contiguous); the NCTHW <-> NDHWC conversion happens once at the module boundary.
 * ===================================================================================================== */

/* ---- CausalConv3d (+ optional fused nearest upsample in front, + optional fused residual add behind).
 * replaces CausalConv3d.forward = F.pad(x, (k/2,k/2,k/2,k/2,k-1,0), "replicate") + ChannelChunkConv3d
 * (hunyuan_vae/unet_causal_3d_blocks.py:82-96; vae/utils.py:153-190 — the channel chunking is unnecessary here:
 * 64-bit addressing), the interpolation of UpsampleCausal3D.forward (unet_causal_3d_blocks.py:136-150: frame 0
 * upsampled in H,W only, later frames in T,H,W) when up_t/up_hw != 0, the strided DownsampleCausal3D conv
 * (:175), the 1x1x1 conv_shortcut / quant_conv / post_quant_conv (ksize 1), and the `input + hidden` of
 * ResnetBlockCausal3D.forward (:257) when res != NULL.
 *   x   bf16 [B, T, H, W, Cin]   source grid BEFORE the virtual upsample; Cin = 8 * 2^j (pad 3 -> 8 channels)
 *   w   bf16 [Cout, w_row_stride], element [co][((dt*3 + dh)*3 + dw)*Cin + ci] = weight[co][ci][dt][dh][dw];
 *       rows zero-padded to w_row_stride >= round_up(ksize^3 * Cin, 64)
 *   bias f32 [Cout] or NULL;  res bf16 [B, To, Ho, Wo, Cout] or NULL;  out bf16 [B, To, Ho, Wo, Cout]
 *   To = (Tu-1)/stride_t + 1 with Tu = up_t ? 1 + 2(T-1) : T;  Ho = (Hu-1)/stride_h + 1 with Hu = up_hw ? 2H : H
 * f32 accumulate, one rounding (bias and residual added in f32).
 * Kernel by shape (same contract for all, chosen inside): 3 x 3 x 3, stride 1, Cin % 128 == 0, Cout >= 128 and whole 16 x 16 output
 * bricks -> the LDS sliding window (the halo brick of a 32-channel block resident in LDS, taps = immediate offsets; with or
 * without the fused upsample; two-frame tiles for Cout == 128); other Cin % 128 == 0, Cout >= 128 shapes -> the table-driven implicit
 * GEMM; Cout <= 4 with Cin == 128 -> a v_dot2_f32_bf16 reduction; everything else -> the 128 x 128 implicit-GEMM tile. */
int osk_causal_conv3d_ndhwc_bf16(const void* x, int B, int T, int H, int W, int Cin,
                                 const void* w, int64_t w_row_stride, const float* bias, int Cout, int ksize,
                                 int stride_t, int stride_h, int stride_w, int up_t, int up_hw,
                                 const void* res, void* out, int To, int Ho, int Wo, void* stream);

/* ---- the same convolution + the GroupNorm statistics of its OUTPUT in the epilogue: the first half of the nn.GroupNorm
 * that consumes this tensor next (ResnetBlockCausal3D.norm2 after conv1, the next block's norm1 / Attention.group_norm /
 * conv_norm_out after conv2 + residual or a Down/Upsample conv: unet_causal_3d_blocks.py:247-259) without the extra
 * read of the tensor that osk_groupnorm_stats_ndhwc_bf16 costs.
 *   gn_sums f64 [B, gn_groups, 2], ZEROED BY THE CALLER; on return (stream order) it holds what
 *   osk_groupnorm_stats_ndhwc_bf16(out, ...) would (sums of the bf16-rounded outputs; f32 partials per 256-voxel tile,
 *   f64 atomics across tiles) -- feed it to osk_groupnorm_apply_ndhwc_bf16.  The waves of a tile add their partials with
 *   LDS float atomics: the result is reproducible to f32 rounding of a tile's partial (~1e-7 relative), not bit for bit.
 * Only the large-tile kernels carry this epilogue: returns OSK_EUNSUPPORTED -- and launches NOTHING -- unless
 * Cin % 128 == 0, Cout >= 128, Cout % 32 == 0, Cout / gn_groups in {4, 8, 16}, >= 256 output voxels, out and res 16-byte aligned and
 * (B == 1 or To*Ho*Wo % 256 == 0); the caller then runs the plain conv + osk_groupnorm_stats_ndhwc_bf16. */
int osk_causal_conv3d_gn_ndhwc_bf16(const void* x, int B, int T, int H, int W, int Cin,
                                    const void* w, int64_t w_row_stride, const float* bias, int Cout, int ksize,
                                    int stride_t, int stride_h, int stride_w, int up_t, int up_hw,
                                    const void* res, void* out, int To, int Ho, int Wo,
                                    double* gn_sums, int gn_groups, void* stream);

/* ---- which kernel serves a causal conv call (host only: launches nothing, needs no device).  The three entry points launch by
 * switching on the value this reports (one selection function, csrc/conv_params.h), so report and launch cannot drift.
 *   the shape arguments of osk_causal_conv3d_ndhwc_bf16;
 *   out_align / res_align: the byte alignment of out / res as a power of two (8, 16, ...; res_align 0 = no residual);
 *   gn_groups > 0: as osk_causal_conv3d_gn_ndhwc_bf16 with that many groups (gn_sums != NULL);  gn_in != 0: as
 *   osk_causal_conv3d_gnin_ndhwc_bf16 (that entry point has no upsample; with up_t or up_hw set the report is OSK_EUNSUPPORTED).
 * Returns the negative status the entry point would return -- OSK_EUNSUPPORTED where gn_sums / gn_in is asked of a shape whose
 * kernel does not carry it, nothing launched -- or OSK_CONV_* | (OSK_CONV_FUSED_STATS when the fused-statistics epilogue is on).
 * The fused statistics need out AND res 16-byte aligned (they ride in the epilogue's 16-byte path). */
#define OSK_CONV_TILE128 0       /* conv3d_kernel<false>: 128 x 128 implicit-GEMM tile, Cin % 64 != 0 */
#define OSK_CONV_TILE128_BIGC 1  /* conv3d_kernel<true>: the same tile, Cin % 64 == 0 */
#define OSK_CONV_FEWOUT 2        /* conv_fewout_kernel<Cout>, Cout <= 4 */
#define OSK_CONV_X4 3            /* conv256x_kernel<4>: 256 voxels x 128 channels, table-driven implicit GEMM */
#define OSK_CONV_X8 4            /* conv256x_kernel<8>: 256 x 256 */
#define OSK_CONV_SW4 5           /* convsw_kernel<4>: sliding window, 128 channels per tile */
#define OSK_CONV_SW8 6           /* convsw_kernel<8>: 256 channels per tile */
#define OSK_CONV_SW4_UP 7        /* convsw_kernel<4, UP>: the nearest upsample folded into the halo */
#define OSK_CONV_SW8_UP 8        /* convsw_kernel<8, UP> */
#define OSK_CONV_SW8_GN 9        /* convsw_kernel<8, false, GN>: input GroupNorm + SiLU folded in */
#define OSK_CONV_SW2 10          /* convsw2_kernel: two-frame tiles, Cout == 128 */
#define OSK_CONV_SW2_GN 11       /* convsw2_kernel<GN> */
#define OSK_CONV_FUSED_STATS 0x100
int osk_causal_conv3d_kernel_class(int B, int T, int H, int W, int Cin, int64_t w_row_stride, int Cout, int ksize,
                                   int stride_t, int stride_h, int stride_w, int up_t, int up_hw, int To, int Ho, int Wo,
                                   int out_align, int res_align, int gn_groups, int gn_in);

/* =====================================================================================================
 * Flux 2-D autoencoder (/root/reference/opensora/models/vae/autoencoder_2d.py, the image stage of the t2i2v pipeline).
 * Activations are NHWC bf16 ([B, H, W, C] contiguous, B = batch x frames as the reference folds T into the batch,
 * autoencoder_2d.py:269-291); the mid attention, GroupNorm and 1x1 projections reuse the entry points of the causal VAE.
 * ===================================================================================================== */

/* ---- zero-padded Conv2d (+ optional fused nearest 2x upsample in front, + optional fused residual add behind).
 * replaces every nn.Conv2d of autoencoder_2d.py: the 3x3 padding=1 convs of ResnetBlock / Upsample / conv_in / conv_out
 * (:80-83,119,149,204,241), the interpolate(scale_factor=2, "nearest") of Upsample.forward (:121) when up != 0, the
 * F.pad(x, (0, 1, 0, 1)) + stride-2 conv of Downsample (:107-113: pad = 0, stride = 2), the 1x1 nin_shortcut (:84) with
 * ksize 1, and the `x + h` of ResnetBlock.forward (:101) when res != NULL.
 *   x   bf16 [B, H, W, Cin]   source grid BEFORE the virtual upsample; Cin = 8 * 2^j (pad 3 -> 8 channels)
 *   w   bf16 [Cout, w_row_stride], element [co][(dh*ksize + dw)*Cin + ci] = weight[co][ci][dh][dw];
 *       rows zero-padded to w_row_stride >= round_up(ksize^2 * Cin, 64)
 *   bias f32 [Cout] or NULL;  res bf16 [B, Ho, Wo, Cout] or NULL;  out bf16 [B, Ho, Wo, Cout]
 *   ksize 1 or 3, stride 1 or 2; `pad` zero rows / columns in front (0 <= pad < ksize); every tap beyond the far edge of the
 *   (upsampled: 2H x 2W) image reads zero as well.  Ho, Wo: the caller's output extent; each output window must start
 *   inside the padded image ((Ho-1)*stride - pad <= Hu-1), so padding=1 -> Ho = Hu, Downsample -> Ho = Hu/2.
 * f32 accumulate, one rounding (bias and residual added in f32).  128 x 128 x 64 implicit-GEMM tile on MFMA (csrc/conv2d.hip);
 * the out-of-image taps are loaded from a zero page.
 *   gn_sums: reserved for GroupNorm statistics of the output in the epilogue, with the contract of
 *   osk_causal_conv3d_gn_ndhwc_bf16.  This kernel has no such epilogue: gn_sums != NULL returns OSK_EUNSUPPORTED and launches
 *   NOTHING (the caller runs the plain conv + osk_groupnorm_stats_ndhwc_bf16). */
int osk_conv2d_nhwc_bf16(const void* x, int B, int H, int W, int Cin, const void* w, int64_t w_row_stride,
                         const float* bias, int Cout, int ksize, int stride, int pad, int up, const void* res,
                         void* out, int Ho, int Wo, double* gn_sums, int gn_groups, void* stream);

/* ---- GroupNorm statistics: sums[b][g] = (sum, sum of squares) in f64 over S voxels x C/G channels.
 * first half of nn.GroupNorm(32, C, eps=1e-6) (unet_causal_3d_blocks.py:216,218; vae.py:115,229; diffusers
 * Attention.group_norm).  x bf16 [B, S, C]; sums f64 [B, G, 2] (zeroed inside, on the stream).  C in
 * {32..512} power of two, C/G <= 16. */
int osk_groupnorm_stats_ndhwc_bf16(const void* x, int B, int64_t S, int C, int G, double* sums, void* stream);

/* ---- GroupNorm apply (+ SiLU): y = bf16((x - mean_g) * rstd_g * gamma_c + beta_c); out = silu ? bf16(y*sigmoid(y)) : y
 * second half of nn.GroupNorm + nonlinearity (unet_causal_3d_blocks.py:250-254).  gamma/beta f32 [C]. */
int osk_groupnorm_apply_ndhwc_bf16(const void* x, const double* sums, const float* gamma, const float* beta,
                                   void* out, int B, int64_t S, int C, int G, float eps, int silu, void* stream);

/* ---- GroupNorm + SiLU folded into the CONSUMING convolution (round 4): the norm1 -> SiLU -> conv1 and norm2 -> SiLU -> conv2
 * chains of ResnetBlockCausal3D.forward (unet_causal_3d_blocks.py:247-256) without the normalised tensor ever existing in HBM.
 * osk_groupnorm_table_f32: sums (osk_groupnorm_stats_ndhwc_bf16 / a producing conv's gn_sums) + gamma, beta ->
 *   table f32 [B][C / 8][16]: per 8-channel chunk 8 scales a_c = rstd_g gamma_c, then 8 shifts d_c = beta_c - mean_g a_c
 *   (exactly the per-channel constants osk_groupnorm_apply_ndhwc_bf16 derives; 16-byte aligned).
 * osk_causal_conv3d_gnin_ndhwc_bf16: osk_causal_conv3d_ndhwc_bf16 (no upsample) of
 *   bf16(silu(bf16(x * a + d))) -- the same rounding points as apply(silu = 1) followed by the conv -- reading x itself: the
 *   sliding-window kernels fetch their halo pieces into registers, transform them in the MFMA shadows and write them to LDS.
 *   gn_sums != NULL: + the fused statistics of the OUTPUT as osk_causal_conv3d_gn_ndhwc_bf16 (gn_groups groups; zeroed by the caller).
 *   Shapes: 3 x 3 x 3, stride 1, Cin % 128 == 0, whole 16 x 16 output bricks, Cout >= 256 or (Cout == 128 and T >= 2); anything
 *   else returns OSK_EUNSUPPORTED and launches NOTHING -- the caller then runs apply + the plain conv. */
int osk_groupnorm_table_f32(const double* sums, const float* gamma, const float* beta, float* table, int B, int64_t S,
                            int C, int G, float eps, void* stream);
int osk_causal_conv3d_gnin_ndhwc_bf16(const void* x, const float* gn_in_table, int B, int T, int H, int W, int Cin,
                                      const void* w, int64_t w_row_stride, const float* bias, int Cout, int ksize,
                                      int stride_t, int stride_h, int stride_w, const void* res, void* out, int To, int Ho,
                                      int Wo, double* gn_sums, int gn_groups, void* stream);

/* ---- frame-causal masked softmax over attention score rows (mid-block attention, one head of dim C):
 *   probs[i][j] = softmax_j(scale * scores[i][j])  over keys j < (i / keys_per_frame + 1) * keys_per_frame,
 *   0 elsewhere (columns up to ld_probs are written, so probs is a K-padded GEMM operand).
 * replaces prepare_causal_attention_mask + the softmax inside diffusers Attention / SDPA
 * (unet_causal_3d_blocks.py:52-60,345-351).  keys_per_frame = 0: no mask.  scores f32, probs bf16. */
int osk_masked_softmax_f32_bf16(const float* scores, int64_t ld_scores, void* probs, int64_t ld_probs,
                                int Sq, int Sk, int keys_per_frame, float scale, void* stream);

/* ---- flash attention of the causal VAE's mid block: ONE head of dimension 512, frame-causal mask
 *   out[i] = softmax_j(scale * q[i].k[j]) v[j]  over keys j with  j / keys_per_frame <= i / keys_per_frame   (+ bias_v)
 * replaces diffusers Attention + prepare_causal_attention_mask inside UNetMidBlockCausal3D
 * (hunyuan_vae/unet_causal_3d_blocks.py:52-60,312-351): no S x S mask, no S x S score matrix in memory.
 * q, k, out: bf16 [B, S, 512] views (batch / row strides in elements, rows contiguous); vt: bf16 V^T [B][512][ld]
 * (natural key order, ld >= round_up(S, 32), ZERO beyond S) -- the layout the V projection GEMM V^T = W_v x^T writes;
 * bias_v f32 [512] | NULL is added after normalisation (softmax rows sum to one).  keys_per_frame = 0: no mask. */
int osk_attention_hd512_fwd_bf16(const void* q, int64_t q_batch_stride, int64_t q_row_stride, const void* k,
                                 int64_t k_batch_stride, int64_t k_row_stride, const void* vt, int64_t vt_batch_stride,
                                 int64_t vt_row_stride, const float* bias_v, void* out, int64_t out_batch_stride,
                                 int64_t out_row_stride, int B, int S, int keys_per_frame, float scale, void* stream);
/* ... with a caller-owned workspace (>= osk_attention_hd512_workspace_bytes(B, S), 16-byte aligned): the launch is only
 * ceil(S / 128) x B x 2 workgroups and its time is the key-tile chain of the last frame's query blocks, so with a workspace every
 * chain is cut into up to 4 runs of key tiles that run side by side (partial rows in f32 + LSE, combined by a merge kernel).
 * Same result up to the f32 rounding of the combination; NULL / too small a workspace = the single-chain launch. */
int osk_attention_hd512_fwd_ws_bf16(const void* q, int64_t q_batch_stride, int64_t q_row_stride, const void* k,
                                    int64_t k_batch_stride, int64_t k_row_stride, const void* vt, int64_t vt_batch_stride,
                                    int64_t vt_row_stride, const float* bias_v, void* out, int64_t out_batch_stride,
                                    int64_t out_row_stride, int B, int S, int keys_per_frame, float scale, void* workspace,
                                    int64_t workspace_bytes, void* stream);
int64_t osk_attention_hd512_workspace_bytes(int B, int S);

/* ---- tile cross-fade of the tiled VAE paths, in place in b (f32 math, one rounding):
 *   b[o, e, i] = a[o, Da - extent + e, i] * (1 - e/extent) + b[o, e, i] * (e/extent),  e < extent
 * replaces blend_v / blend_h / blend_t (hunyuan_vae/autoencoder_kl_causal_3d.py:360-382; a Python loop of `extent`
 * slice assignments there).  a, b: contiguous bf16 viewed as [outer, Da | Db, inner] along the blended axis
 * (NCTHW tiles: blend_t -> outer B*C, inner H*W; blend_v -> outer B*C*T, inner W; blend_h -> outer B*C*T*H, inner 1). */
int osk_blend_bf16(const void* a, void* b, int64_t outer, int Da, int Db, int extent, int64_t inner, void* stream);

/* =====================================================================================================
 * Video DC-AE decoder and encoder (/root/reference/opensora/models/dc_ae, "dc-ae-f32t4c128": the autoencoder of
 * configs/diffusion/inference/high_compression.py).  Activations are NDHWC bf16 ([B, T, H, W, C] contiguous); the 1x1x1
 * convolutions without an activation are osk_gemm_bf16 over the B*T*H*W rows.  (Added without changing any existing contract:
 * the version stays 2.)  csrc/dc_ae.hip.
 * ===================================================================================================== */

/* ---- zero-padded Conv3d, stride 1, "same" padding in T, H and W (+ nearest upsample in front, + SiLU, + residual add behind).
 * replaces ConvLayer(is_video=True) of dc_ae/models/nn/ops.py:56-136 -- F.pad(x, (k/2,)*6, "constant") + ChannelChunkConv3d
 * (:87-96,130-131) and its act (:134-135) -- for every dense conv of the decoder: project_in (dc_ae.py:314-324), the
 * InterpolateConvUpSampleLayer convs with their chunked_interpolate(scale_factor=[1|2, 2, 2], "nearest") in front (ops.py:285-295:
 * up_t, up_hw), ResBlock conv1 (+ SiLU) / conv2 (ops.py:615-639), project_out's conv (dc_ae.py:352-362), the 1x1x1
 * GLUMBConv.inverted_conv (+ SiLU, ops.py:552-560), and the `main + shortcut` of ResidualBlock.forward (ops.py:923) when res != NULL.
 *   x   bf16 [B, T, H, W, Cin]  source grid BEFORE the virtual upsample; Cin = 8 * 2^j
 *   w   bf16 [Cout, w_row_stride], element [co][((dt*k + dh)*k + dw)*Cin + ci] = weight[co][ci][dt][dh][dw];
 *       rows zero-padded to w_row_stride >= round_up(k^3 * Cin, 64)
 *   bias f32 [Cout] | NULL;  res bf16 like out | NULL;  out bf16 [B, T << up_t, H << up_hw, W << up_hw, Cout]
 *   out = bf16( act(acc + bias) + res ), act = SiLU when act != 0; f32 accumulate, one rounding.
 * 128 x 128 x 64 implicit-GEMM tile on MFMA, out-of-volume taps loaded from a zero page; any Cout >= 1 (Cout = 3 runs on the
 * same tile with 3 live columns).  Cin not 8 * 2^j or a volume beyond 2^31 voxels: OSK_EUNSUPPORTED, nothing launched. */
int osk_conv3d_zp_ndhwc_bf16(const void* x, int B, int T, int H, int W, int Cin, const void* w, int64_t w_row_stride,
                             const float* bias, int Cout, int ksize, int up_t, int up_hw, int act, const void* res,
                             void* out, void* stream);

/* ---- zero-padded strided Conv3d of the encoder's downsample blocks (+ residual add behind).
 * replaces ConvLayer(is_video=True, kernel_size=3, stride=(1|2, 2, 2), use_bias=True, norm=None, act_func=None) as
 * build_downsample_block builds it (dc_ae.py:166-195) -- F.pad(x, (1,)*6, "constant") + ChannelChunkConv3d(stride) (ops.py:87-106,
 * 130-131) -- and the `main + shortcut` of ResidualBlock.forward (ops.py:923) when res != NULL.
 *   x   bf16 [B, T, H, W, Cin], Cin = 8 * 2^j;  w, w_row_stride, bias as for osk_conv3d_zp_ndhwc_bf16 with k = 3
 *   stride_t 1 | 2, stride_hw == 2 (anything else: OSK_EINVAL)
 *   out bf16 [B, (T-1)/stride_t + 1, (H-1)/2 + 1, (W-1)/2 + 1, Cout] (PyTorch's floor((n + 2 - 3)/s) + 1);  res like out | NULL
 *   out[b, to, ho, wo] = bf16( sum_taps w . x[b, to*stride_t - 1 + dt, ho*2 - 1 + dh, wo*2 - 1 + dw] + bias + res ), taps outside
 *   the volume of batch b are zeros; f32 accumulate, one rounding, no activation.  Odd T, H, W are legal (there the far padding
 *   is read); stride_t = 2 with T = 1 yields one frame from the taps (pad, frame, pad).
 * The tile, alignment rules, limits and error codes of osk_conv3d_zp_ndhwc_bf16. */
int osk_conv3d_zp_strided_ndhwc_bf16(const void* x, int B, int T, int H, int W, int Cin, const void* w, int64_t w_row_stride,
                                     const float* bias, int Cout, int stride_t, int stride_hw, const void* res, void* out,
                                     void* stream);

/* ---- pixel-unshuffle channel averaging: the shortcut of the encoder's downsample blocks and of its project_out.
 * replaces PixelUnshuffleChannelAveragingDownSampleLayer.forward (ops.py:189-228): pixel_unshuffle_3d (vo_ops.py:38-56; ft = fhw = 2),
 * or F.pixel_unshuffle on H, W only (no temporal downsample or T == 1, ops.py:217-222; ft = 1, fhw = 2), or the factor-1 form of
 * project_out (ft = fhw = 1), then view(B, Cout, gs, ...).mean(2).  per = ft * fhw^2, gs = Cin * per / Cout (must divide):
 *   out[b, t, h, w, co] = bf16( (1/gs) * sum_{g < gs} x[b, t*ft + dt, h*fhw + dh, w*fhw + dw, c] ),
 *   u = co*gs + g, c = u / per, s = u % per, dt = s / fhw^2, dh = (s / fhw) % fhw, dw = s % fhw.
 * x bf16 [B, T, H, W, Cin]; out bf16 [B, T/ft, H/fhw, W/fhw, Cout].  f32 sum, one rounding.  A gather, HBM bound.
 * T % ft, H % fhw, W % fhw or Cin * per % Cout != 0: OSK_EINVAL;  Cout % 8 != 0: OSK_EUNSUPPORTED; nothing launched. */
int osk_unshuffle_avg_ndhwc_bf16(const void* x, int B, int T, int H, int W, int Cin, void* out, int Cout, int ft, int fhw,
                                 void* stream);

/* ---- channel-duplicating pixel shuffle: the shortcut of the upsample blocks and of project_in.
 * replaces ChannelDuplicatingPixelShuffleUpSampleLayer.forward (ops.py:316-337): repeat_interleave(rep, dim=1) + pixel_shuffle_3d
 * (vo_ops.py:11-35; ft = fhw = 2), + F.pixel_shuffle on H, W only (the T == 1 / no temporal upsample branch, ops.py:333-336;
 * ft = 1, fhw = 2), + the factor-1 form of project_in (ft = fhw = 1), rep = Cout * ft * fhw^2 / Cin (must divide):
 *   out[b, t, h, w, co] = x[b, t / ft, h / fhw, w / fhw, (((co*ft + t % ft)*fhw + h % fhw)*fhw + w % fhw) / rep]
 * x bf16 [B, T, H, W, Cin]; out bf16 [B, T*ft, H*fhw, W*fhw, Cout], Cout % 8 == 0.  A gather, HBM bound. */
int osk_dup_shuffle_ndhwc_bf16(const void* x, int B, int T, int H, int W, int Cin, void* out, int Cout, int ft, int fhw,
                               void* stream);

/* ---- depthwise Conv3d, k = 3 or 5, zero "same" padding, + bias, + GLU.
 * replaces GLUMBConv.depth_conv and the chunk / silu / multiply behind it (ops.py:561-571,584-588; glu != 0: out has C / 2 channels,
 * out[c] = (y[c] + b[c]) * silu(y[c + C/2] + b[c + C/2])) and LiteMLA.aggreg[0][0] (ops.py:684-691; k = 5, no bias, glu = 0).
 *   x bf16 [B, T, H, W, C];  w bf16 [k^3, C], element [(dt*k + dh)*k + dw][c] = weight[c][0][dt][dh][dw];  bias f32 [C] | NULL
 * f32 accumulate, one rounding.  C % 8 (glu: % 16) != 0 or another k: OSK_EUNSUPPORTED. */
int osk_dwconv3d_ndhwc_bf16(const void* x, int B, int T, int H, int W, int C, const void* w, const float* bias, int ksize,
                            int glu, void* out, void* stream);

/* ---- block-diagonal 1x1x1 conv, 32 -> 32 channels per group, no bias.
 * replaces LiteMLA.aggreg[0][1] (ops.py:692: groups = 3 * heads, dim 32).  x, out bf16 [M, C]; w bf16 [C, 32] =
 * weight[co][ci] (ci within co's group).  MFMA, f32 accumulate.  C % 32 != 0: OSK_EUNSUPPORTED. */
int osk_gconv32_bf16(const void* x, int64_t M, int C, const void* w, void* out, void* stream);

/* ---- ReLU linear attention, head dim 32.
 * replaces LiteMLA.relu_linear_att (ops.py:709-765).  qkv bf16 [B, N, G * 96]: G consecutive [q | k | v] groups of 3 x 32
 * channels.  Per (b, g):  KV = sum_n [v_n ; 1] relu(k_n)^T  (33 x 32),  o_n = KV relu(q_n),  out_n = o_n[:32] / (o_n[32] + eps).
 * out bf16: row (b, n) at out + (b*N + n) * out_row_stride, columns g*32 .. g*32 + 31 (so two scales write one [.., 2C] tensor).
 * All sums in f32.  workspace: f32, >= B * G * nsplit * 1056 * 4 bytes; the tokens are cut into nsplit runs whose partial KV are
 * summed in a fixed order (deterministic).  B * G > 65535 or nsplit > 1024: OSK_EUNSUPPORTED. */
int osk_relu_linear_attn_bf16(const void* qkv, int B, int N, int G, void* out, int64_t out_row_stride, float* workspace,
                              int64_t workspace_bytes, int nsplit, float eps, void* stream);

/* ---- RMSNorm over channels with affine weight and bias (+ ReLU, + shortcut add).
 * replaces RMSNorm3d.forward (dc_ae/models/nn/norm.py:63-68, eps 1e-5), the ReLU behind project_out's norm (dc_ae.py:346-349)
 * when relu != 0, and the identity-shortcut add of ResidualBlock.forward (ops.py:923) when res != NULL:
 *   out = act(x * rsqrt(mean_c(x^2) + eps) * weight + bias) + res.   x, res, out bf16 [M, C]; weight, bias f32 [C]; C % 8 == 0.
 * f32 statistics, one rounding. */
int osk_rmsnorm_affine_bf16(const void* x, int64_t M, int C, const float* weight, const float* bias, float eps,
                            const void* res, int relu, void* out, void* stream);

/* ==== CLIP-L text encoder: the three entries below replace the arithmetic inside the Hugging Face CLIPTextModel that HFEmbedder
 * runs for `y_vec` (opensora/models/text/conditioner.py:17-20 builds it, 48-53 calls it: 77 tokens, attention_mask=None,
 * `pooler_output`).  open_sora_amd/clip.py is their caller. */

/* ---- LayerNorm over channels with affine weight and bias (nn.LayerNorm: CLIPEncoderLayer.layer_norm1 / layer_norm2 and
 * final_layer_norm).
 * replaces the nn.LayerNorm calls of the CLIP branch (conditioner.py:17-20, 48-53):
 *   out[m, :] = bf16((x[m, :] - mean) * rsqrt(var + eps) * weight + bias),   var = mean((x - mean)^2)   (biased)
 * x, out bf16 [M, C], rows x_row_stride / out_row_stride elements apart (% 8 == 0, >= C), 16-byte aligned; weight, bias f32 [C].
 * f32 statistics over the register-resident row, the mean first and then the variance of the centred values (never
 * E[x^2] - mean^2: a constant row comes out as bf16(bias), not NaN); one rounding.  C % 8 == 0 and C <= 4096; another C:
 * OSK_EUNSUPPORTED, nothing launched. */
int osk_layernorm_affine_bf16(const void* x, int64_t x_row_stride, void* out, int64_t out_row_stride, const float* weight,
                              const float* bias, int64_t M, int C, float eps, void* stream);

/* ---- causal softmax self-attention, head dim 64: the attention of the CLIP text tower.
 * replaces CLIPAttention.forward under the causal mask of CLIPTextTransformer (conditioner.py:17-20, 48-53):
 *   out[b, i, h] = sum_{j <= i} softmax_j(scale * q_i . k_j) v_j ,   Lq = Lk = L
 * Operands as osk_attention_relbias_bf16 (q, k, v, out bf16 [B, L, H * hd] views with batch / row strides in elements; q | k | v may
 * be read in place from one fused projection output; V as stored), no bias argument.  The CAUSAL instantiation of that kernel:
 * query block qb walks key tiles 0 .. qb only (tiles above the diagonal are skipped, not masked), the diagonal tile masks j > i
 * with -inf before the running maximum.  hd == 64 and 1 <= L <= 4096; another hd or a longer L: OSK_EUNSUPPORTED, nothing written. */
int osk_attention_causal_bf16(const void* q, int64_t q_batch_stride, int64_t q_row_stride, const void* k, int64_t k_batch_stride,
                              int64_t k_row_stride, const void* v, int64_t v_batch_stride, int64_t v_row_stride, void* out,
                              int64_t o_batch_stride, int64_t o_row_stride, int B, int H, int L, int hd, float scale, void* stream);

/* ---- Linear + quick-GELU: CLIPMLP.fc1 and its activation.
 * replaces fc1 + QuickGELUActivation of the CLIP branch (conditioner.py:17-20, 48-53):
 *   C = bf16(quick_gelu(A W^T + bias)),   quick_gelu(v) = v * sigmoid(1.702 v) = v / (1 + exp2(-1.702 log2(e) v))  in f32
 * The arguments of osk_gemm_bf16 without res / gate / gelu_from / out_f32 (C is bf16), the same constraints (K % 64 == 0, strides,
 * alignment).  ALWAYS the 128 x 128 tile kernel, whatever M: at large M it runs at about half the rate of the 256-row tiles
 * osk_gemm_bf16 would pick.  CLIP never has large M (3 x 77 rows); the large-tile epilogues know no quick-GELU. */
int osk_gemm_quickgelu_bf16(const void* A, int64_t a_batch_stride, int64_t a_row_stride, int a_rows_per_batch, const void* W,
                            int64_t w_row_stride, const float* bias, void* C, int64_t c_batch_stride, int64_t c_row_stride,
                            int c_rows_per_batch, int M, int N, int K, void* stream);

/* ---- LoRA adapters merged into a Linear weight, on the device, at plan-build time.
 * replaces the peft wrapping of the MMDiT in prepare_api (opensora/utils/sampling.py:542-545: `pretrained_lora_path` ->
 * PeftModel.from_pretrained(model, path, is_trainable=False)), for the adapters the trainer writes (scripts/diffusion/train.py:208-216,
 * opensora/utils/ckpt.py:421-422) on the Linear layers of the double / single blocks (opensora/models/mmdit/model.py:198):
 *   out[n, k] = bf16_rne( f32(w[n, k]) + sum_i scale_i * sum_j B_i[n, j] * A_i[j, k] ),      n < N, k < K
 * w, out bf16 [N, K] with rows w_row_stride / out_row_stride elements apart (>= K, % 8 == 0, base pointers 16-byte aligned): a row
 * slice of a concatenated weight (q_proj | k_proj | v_proj) is merged in place through its stride.  out may be w itself (same pointer
 * and stride); any other overlap of the two is undefined.  Nothing outside the [N, K] window is read or written.
 * Adapter i: A_i bf16 [r, K] (lora_A.weight; rows a_row_stride apart, >= K, % 8 == 0, 16-byte aligned), B_i bf16 [N, r]
 * (lora_B.weight; rows b_row_stride apart, >= r, any alignment), 1 <= r <= 256 arbitrary (padded with zeros inside the kernel),
 * scale finite (lora_alpha / r times the adapter's weight; may be negative or zero).  `adapters` is a HOST array, read before the
 * call returns.  0 <= n_adapters <= 8; with 0 the call is a strided copy, bit for bit.
 * The bf16 x bf16 products are exact in f32 and every sum is kept in f32 (MFMA accumulation over the rank per adapter, one fma per
 * adapter by its scale, W added last): ONE rounding to bf16, not one per adapter.  A delta below half a bf16 ulp of w[n, k] is lost.
 * N >= 1 arbitrary, K % 8 == 0.  No allocation, no synchronisation: may be captured in a hipGraph. */
typedef struct OskLoraAdapter {
  const void* a; int64_t a_row_stride;
  const void* b; int64_t b_row_stride;
  int r; float scale;
} OskLoraAdapter;
int osk_lora_merge_bf16(const void* w, int64_t w_row_stride, void* out, int64_t out_row_stride, int N, int K,
                        const OskLoraAdapter* adapters, int n_adapters, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* OSK_H */
