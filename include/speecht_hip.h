/* speecht_hip.h -- C ABI of libspeecht_hip.so: the MI355X (gfx950) kernels behind the
 * speechT Wav2Letter training / inference step.
 *
 * The reference (louiskirsch/speechT) has no FFI of its own: its hot path is a list of
 * TensorFlow-1 / librosa op call sites.  Each entry point below replaces one of those call
 * sites (file:line relative to the reference root) and is what a reference-side ctypes
 * binding would bind (INTEGRATION.md shows the stub).  Conventions:
 *   - plain `extern "C"`, pointers + sizes only, no torch / C++ types;
 *   - every pointer is a caller-owned DEVICE pointer unless the name says `host_`;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); calls only enqueue
 *     work, they never synchronise and never allocate;
 *   - return 0 on success, a negative ST_E* code otherwise; st_last_error() gives the text
 *     (thread-local);
 *   - workspaces are explicit: query the size, pass the buffer.
 *
 * Activation layout ("padded NWC"): the reference's (batch, time, channel) tensors
 * (speech_model.py:44) are stored with zero halo rows around every utterance and the channel
 * pitch rounded up to 16 floats, so that tf.nn.conv1d's SAME padding (speech_model.py:155)
 * becomes plain in-bounds reads and every im2col row is one contiguous, 64-byte aligned span.
 */
#ifndef SPEECHT_HIP_H
#define SPEECHT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ST_OK 0
#define ST_EINVAL (-1)   /* bad argument / layout precondition violated */
#define ST_ELAUNCH (-2)  /* HIP launch error */
#define ST_EWORKSPACE (-3)
#define ST_ECOMM (-4)    /* RCCL unavailable or a collective failed */

/* element (b, t, c) lives at base[((int64)b * t_pitch + halo + t) * c_pitch + c];
 * rows outside [0, frames) and channels in [channels, c_pitch) must hold zeros. */
typedef struct st_tensor3 {
  float* base;
  int32_t batch;
  int32_t frames;
  int32_t channels;
  int32_t halo;     /* zero rows in front of frame 0 */
  int32_t t_pitch;  /* rows per utterance, halo + frames + trailing zero rows */
  int32_t c_pitch;  /* floats per row, multiple of 16 */
} st_tensor3;

int st_version(void);
const char* st_last_error(void);

/* ---- diagnostics (no reference counterpart) ----------------------------------------------
 * Launch trace: between st_trace_begin() and st_trace_end() every entry point appends one text line per
 * kernel launch naming the variant and split policy it chose (e.g. "gemm_nn<128,128,2,2,fast> epi=1
 * splits=2 M=16032 Np=256 Kp=64512").  st_trace_end copies the text to a HOST buffer (truncating) and
 * returns the bytes needed including the terminator.  Used by the parity tests to assert which kernels a
 * full-size step really ran.  Every line of a matrix-pipe launch carries "gflop=<executed GFLOP, padding included>".
 * st_trace_begin_timed() additionally launches every traced kernel through hipExtLaunchKernel with a start and a stop
 * event (the dispatch's own begin / end time stamps, as a profiler's kernel trace shows them; no marker between
 * launches); st_trace_end then waits for them and appends " ms=<duration>" to each line -- per-launch times INSIDE the
 * real launch sequence of a step, side streams and all (bench.py's in-step roofline).
 * st_set_tuning forces a form the library's policy picks on other shapes (tests, A/B runs); value 0 restores the policy:
 *   "streamk"             1: the per-bin products as the persistent stream-K launch wherever the shape allows, 2: never
 *   "streamk_slots"       64 / 96: workgroups per XCD of that launch
 *   "streamk_test_drop"   1: its producers publish a wrong epoch, so every hand-off is lost (the timeout path)
 *   "no_fused_transforms" 1: the frequency-domain layers' transforms as separate kernels, never fused with a neighbour's
 *   "bf16_lag_copies"     1: the bf16 lag products from transposed copies of the spectra instead of transposing reads
 *   "filters_idft_valu"   1: the filter gradient's inverse transform on the vector ALU instead of the matrix pipe
 *   "bf16_taps_panel"     1: the bf16 W-tap layers on the general kernel instead of conv_taps_bf16
 *   "no_g3"               1: the wide layer's per-bin products in four real products instead of three
 *   "g3_tile"             1: 64-row tiles, 2: 128-row tiles, 4: 64-row tiles and the reduction split in two (three-product kernels)
 * Any other name fails with ST_EINVAL.  The launch path never reads the environment. */
int st_trace_begin(void);
int st_trace_begin_timed(void);
/* Timed mode only times the launches whose trace line contains `text` (NULL or "": all).  A timed launch costs the stream
 * ~7 us (hipExtLaunchKernel with events gives up the back-to-back dispatch), so timing ONE kernel's ten launches per step
 * leaves the step as it is (+1 %), timing all ~100 stretches it by 10 %. */
int st_trace_timed_filter(const char* text);
size_t st_trace_end(char* host_buf, size_t capacity);
int st_set_tuning(const char* name, int value);
/* CRC-32C of a HOST buffer, continuing from `crc` (0 to start): the checksum TensorFlow's checkpoint bundles carry
 * (speech_model.py:122 tf.train.Saver; read and written by speecht_amd/tf_checkpoint.py). */
uint32_t st_host_crc32c(const void* host_data, size_t n, uint32_t crc);

/* ---- filter packing -------------------------------------------------------------------
 * Reference filters are [W, Cin, Cout] (speech_model.py:148-151; the `export --weights`
 * layout, exporting.py:30-40).  The kernels use the row-major GEMM operand
 * packed[k_pad][n_pad], k = w * cin_pitch + c, zero in all padding. */
int st_packed_dims(int width, int cin_pitch, int cout, int* k_valid, int* k_pad, int* n_pad);
int st_pack_filters_f32(const float* filters, int width, int cin, int cout, int cin_pitch,
                        float* packed, void* stream);
int st_unpack_filters_f32(const float* packed, int width, int cin, int cout, int cin_pitch,
                          float* filters, void* stream);
/* packedT[(w' * cout_pitch + o)][c] = packed[((W-1-w') * cin_pitch + c)][o]: the operand that
 * turns back-prop to the layer input into the same implicit-GEMM convolution. */
int st_filters_flip_transpose_f32(const float* packed, int width, int cin, int cout,
                                  int cin_pitch, int cout_pitch, float* packed_t, void* stream);

/* ---- K5-K7: tf.nn.conv1d('SAME') + bias_add + relu (speech_model.py:155,173,177) -------
 * y[b,t,o] = act(bias[o] + sum_{w,c} x[b, t*stride + w - pad_left, c] * F[w,c,o]).
 * Requires x->halo >= pad_left and enough trailing halo; bias has n_pad floats. */
int st_conv1d_nwc_fwd_f32(const st_tensor3* x, const float* packed, const float* bias, int width,
                          int stride, int pad_left, int relu, const st_tensor3* y, void* stream);
/* Same, with a workspace (st_conv1d_fwd_ws bytes; 0 when the shape does not split).  With few output rows
 * (live / single-utterance inference) the reduction is split over the idle CUs and summed in a fixed
 * order; without a large enough workspace the call is identical to st_conv1d_nwc_fwd_f32. */
size_t st_conv1d_fwd_ws(const st_tensor3* x, const st_tensor3* y, int width);
int st_conv1d_nwc_fwd_ws_f32(const st_tensor3* x, const float* packed, const float* bias, int width,
                             int stride, int pad_left, int relu, const st_tensor3* y, void* workspace,
                             size_t workspace_bytes, void* stream);

/* ---- frequency-domain form of the same three operations (csrc/conv_fft.hip) ---------------------------------
 * Time is cut into blocks of 64 frames, every block is taken to the frequency domain by a length-(63 + W) DFT, the W
 * taps become one complex channel-contraction per frequency bin -- run as real GEMMs on the exact-fp32 MFMA kernel --
 * and the result comes back by an inverse DFT fused with the bias / ReLU / mask epilogue: for the model's 32-tap
 * 250 -> 2000 layer (speech_model.py:285; 66 % of the step's MACs) ~10x fewer multiplications than the W-tap form,
 * same fp32 arithmetic class (tests/test_gpu_fft_conv.py).  stride 1, 2 <= W <= 32 (a window of 63 + W frames must not have more than 48 bins); the output channels must pack to a
 * multiple of 128 (and the input channels too for back-prop to the input).  A stride-2 layer of even-ish width runs
 * through the same entry points on its polyphase view: the input read as [B][T/2][2 * c_pitch] (frame pairs as
 * channels), W/2 + 1 taps, the packed filters shifted by one c_pitch block (engine.py does this for
 * the model's first layer).
 *   tables    st_conv1d_fft_table_floats() floats, filled once per (width, pad_left) by st_conv1d_fft_tables_f32
 *   gfwd      the filter spectra as a GEMM operand (st_conv1d_fft_filter_floats floats), rebuilt by
 *             st_conv1d_fft_filters_f32 whenever the weights change; the forward pass multiplies by it, back-prop to the
 *             input by its transpose (read in place: no second set of spectra, no flipped copy of the weights)
 *   sf        spectra of the layer input (st_conv1d_fft_sf_floats floats), written by the forward call and read by
 *             the filter-gradient call
 *   zf        spectra of the gradient wrt the layer output (st_conv1d_fft_zf_floats floats), written by
 *             st_conv1d_fft_dz_spectra_f32, read by both gradient calls
 *   workspace st_conv1d_fft_ws bytes, scratch of one call, headed by st_gemm_nn_batched_ws_f32's area (one workspace per stream)
 * What the calls expect of their buffers: gfwd, sf, zf and the workspace may hold ANY content (every element that is read has been
 * written by the call that owns it: pad rows and pad channels of the spectra as zeros); the halos of the tensors hold zeros
 * (st_zero_halos_f32) and are not written, the interiors of y and dx are written whole, pad channels as zeros.  The filter
 * gradient writes rows [0, width * cin_pitch) of dpacked [k_pad][n_pad], padding as zeros; rows [width * cin_pitch, k_pad) -- there
 * are some when width * cin_pitch is no multiple of 32 -- are NOT written and stay the caller's: zero, like all padding of the
 * packed layout (the engine's gradient buffer is zero-initialised once and nothing ever writes those rows). */
int st_conv1d_fft_plan(int width, int frames, int batch, int* n, int* valid, int* blocks, int* bins, int* rows_pad);
/* the per-bin products themselves: `batches` independent row-major fp32 GEMMs C[i] = A[i] * B[i] (A [m][lda], B [k][n],
 * C [m][ldc]; k a multiple of 32, n of 128; strides in floats) on the convolution MFMA kernel, bin i on XCD i % 8 */
int st_gemm_nn_batched_f32(const float* a, int64_t lda, int64_t a_batch, const float* b, int64_t b_batch, float* c,
                           int64_t ldc, int64_t c_batch, int m, int k, int n, int batches, void* stream);
/* The same with st_gemm_nn_batched_ws_bytes() bytes of scratch: a launch whose 64 x 128 tiles would load the CUs unevenly
 * (the 7-tap layers: 36 bins x 16 tiles = 576 workgroups, three on a quarter of the CUs, two on the rest) then runs as ONE
 * persistent launch that deals the (bin, tile, k-tile) list in equal runs to 512 (or 768) workgroups; a tile cut into pieces
 * is summed head + next + ... by the workgroup that holds its start (bit-reproducible, no atomics on data).  The scratch may
 * hold any content (its first st_gemm_nn_batched_ctrl_bytes() bytes are flags tagged with a per-launch epoch and reset by
 * their reader); one scratch per stream.  The frequency-domain entry points below carry this area at the head of their
 * workspace. */
size_t st_gemm_nn_batched_ws_bytes(void);
size_t st_gemm_nn_batched_ctrl_bytes(void);
/* Lost hand-offs of the persistent launches since the library was loaded.  A reader whose bounded poll runs out (a producer
 * workgroup that never published its partial tile) writes NaN into its tile -- never a sum with an unpublished partial -- and
 * counts here.  st_streamk_lost_ptr: the device address of the 32-bit count; st_streamk_lost_count: a synchronous read (default
 * stream); st_streamk_lost_fetch_async: for a caller that already copies status words back after a step (engine.fetch_losses). */
int st_streamk_lost_ptr(void** device_word);
int st_streamk_lost_count(unsigned* count);
/* the count copied to `host_word` (pinned host memory) behind everything enqueued on `stream` so far */
int st_streamk_lost_fetch_async(unsigned* host_word, void* stream);
int st_gemm_nn_batched_ws_f32(const float* a, int64_t lda, int64_t a_batch, const float* b, int64_t b_batch, float* c,
                              int64_t ldc, int64_t c_batch, int m, int k, int n, int batches, void* workspace,
                              size_t workspace_bytes, void* stream);
/* C[i] = A[i] * Bt[i]^T with the second operand given TRANSPOSED, Bt [n][k] (k contiguous): the products of back-prop to the
 * input, which read the forward filter spectra in place (X = Z gfwd^T) */
int st_gemm_nn_batched_bt_ws_f32(const float* a, int64_t lda, int64_t a_batch, const float* bt, int64_t bt_batch, float* c,
                                 int64_t ldc, int64_t c_batch, int m, int k, int n, int batches, void* workspace,
                                 size_t workspace_bytes, void* stream);
/* out[i] = A[i]^T * Z[i]: A [m][lda] (k columns), Z [m][ldz] (n columns), out [k][n]; the reduction runs over the m rows
 * (m a multiple of 32, k and n of 128) -- the lag products of the filter gradient */
int st_gemm_tn_batched_f32(const float* a, int64_t lda, int64_t a_batch, const float* z, int64_t ldz, int64_t z_batch,
                           float* out, int64_t out_batch, int m, int k, int n, int batches, void* stream);
/* ... with the second operand SHARED by groups of 2^z_batch_shift consecutive products (product b reads Z of batch
 * b >> z_batch_shift): the real and the imaginary lag products of a bin -- over the input spectra and their rotated copy,
 * rows read at half length -- both against that bin's gradient spectra */
int st_gemm_tn_batched_shared_f32(const float* a, int64_t lda, int64_t a_batch, const float* z, int64_t ldz, int64_t z_batch,
                                  float* out, int64_t out_batch, int m, int k, int n, int batches, int z_batch_shift, void* stream);
/* ... on output tiles of 128 x tile_n, tile_n 128 or 64 (the entry points above choose by shape: 64 for a short reduction
 * whose 128-wide tiles are little more than one per CU -- the 7-tap layers; the same bits either way) */
int st_gemm_tn_batched_tile_f32(const float* a, int64_t lda, int64_t a_batch, const float* z, int64_t ldz, int64_t z_batch,
                                float* out, int64_t out_batch, int m, int k, int n, int batches, int z_batch_shift, int tile_n,
                                void* stream);
/* A bin's COMPLEX product in three real products instead of four (Gauss: (a + ib)(c + id) = (k1 - k3) + i (k1 + k2), k1 = c (a + b),
 * k2 = a (d - c), k3 = b (c + d)), the shared product computed once per output tile (round 6; the 32-tap layer's per-bin products,
 * 25 % fewer multiplications).  Operand planes A_p = a + a_off[p], B_p = b + b_off[p] (p = 0, 1, 2; offsets in floats; b rows ldb
 * apart, or with b_transposed != 0 the planes hold B_p^T, [n][ldb]):
 *     c[i][row][col]          = A_0 B_0 + A_1 B_1          c[i][row][c_off2 + col] = A_0 B_0 + A_2 B_2
 * k = reduction length of ONE product (a multiple of 64), n a multiple of 128.  The sums and signs live in the planes: the
 * transforms write [S_r + S_i | S_i | S_r | S_i - S_r] / [Z_r + Z_i | Z_r | Z_i] rows, the filter spectra are the planes
 * G_r, G_i - G_r, -(G_r + G_i) (st_conv1d_fft_three_products says which layers: conv_fft.hip g3_form). */
int st_gemm_nn_g3_batched_f32(const float* a, int64_t lda, int64_t a_batch, const int64_t* a_off, const float* b, int64_t ldb,
                              int64_t b_batch, const int64_t* b_off, int b_transposed, float* c, int64_t ldc, int64_t c_batch,
                              int64_t c_off2, int m, int k, int n, int batches, void* stream);
/* ... and the lag products of the filter gradient: out[i] = A_0^T Z_0 + A_1^T Z_1 and, out_part floats behind it,
 * A_2^T Z_2 - A_0^T Z_0 ([k][n] each), the reduction over the m rows (m a multiple of 32, k and n of 128) */
int st_gemm_tn_g3_batched_f32(const float* a, int64_t lda, int64_t a_batch, const int64_t* a_off, const float* z, int64_t ldz,
                              int64_t z_batch, const int64_t* z_off, float* out, int64_t out_batch, int64_t out_part, int m, int k,
                              int n, int batches, void* stream);
/* which form a frequency-domain layer's per-bin products take: 0 four real products; 2 three (its sf / zf / gfwd buffers then
 * hold the layouts above -- same sizes from the st_conv1d_fft_*_floats functions); 1 three-part gradient spectra rows read by the
 * four-product kernels (an input whose spectra do not tile the three-product kernels).  st_set_tuning("no_g3", 1): always 0. */
int st_conv1d_fft_three_products(int width, int cin_pitch, int cout);
size_t st_conv1d_fft_table_floats(void);
int st_conv1d_fft_tables_f32(int width, int pad_left, float* tables, size_t table_floats, void* stream);
size_t st_conv1d_fft_filter_floats(int width, int cin_pitch, int cout);
int st_conv1d_fft_filters_f32(const float* packed, int width, int cin, int cout, int cin_pitch, const float* tables, float* gfwd,
                              void* stream);
size_t st_conv1d_fft_sf_floats(const st_tensor3* x, const st_tensor3* y, int width);
size_t st_conv1d_fft_zf_floats(const st_tensor3* dz, int width);
size_t st_conv1d_fft_ws(const st_tensor3* x, const st_tensor3* y, int width);
int st_conv1d_nwc_fwd_fft_f32(const st_tensor3* x, const float* gfwd, const float* bias, int width, int pad_left, int relu,
                              const st_tensor3* y, const float* tables, float* sf, void* workspace,
                              size_t workspace_bytes, void* stream);
/* The same for a CHAIN of frequency-domain layers (round 4): sf_ready != 0 -- `sf` already holds this layer's input spectra (the
 * previous layer's call wrote them); next_tables / next_sf / next_width / next_pad_left -- the next layer of the chain: when the
 * shapes allow (at most 8 blocks of 64 frames per utterance, batch x blocks a multiple of 128, the next layer's window reaching at
 * most 4 frames into either neighbour block: the model's 7-tap layers at utterances of up to 10.2 s) the inverse transform hands its
 * frames to the next layer's forward transform in registers and writes next_sf; *next_sf_written says whether it did. */
int st_conv1d_nwc_fwd_fft_chain_f32(const st_tensor3* x, const float* gfwd, const float* bias, int width, int pad_left, int relu,
                                    const st_tensor3* y, const float* tables, float* sf, int sf_ready, const float* next_tables,
                                    float* next_sf, int next_width, int next_pad_left, int* next_sf_written, void* workspace,
                                    size_t workspace_bytes, void* stream);
int st_conv1d_fft_dz_spectra_f32(const st_tensor3* dz, int width, const float* tables, float* zf, void* stream);
/* dbias[o] = sum_{b,t} dz[b,t,o] read off bin 0 of the spectra zf (npad floats written, pads zero): the bias gradient of a
 * frequency-domain layer without another pass over dz */
int st_conv1d_fft_bias_grad_f32(const st_tensor3* dz, int width, const float* zf, float* dbias, void* stream);
int st_conv1d_nwc_bwd_data_fft_f32(const st_tensor3* dz, const float* zf, const float* gfwd, int width, int pad_left,
                                   const st_tensor3* act, const st_tensor3* dx, const float* tables, void* workspace,
                                   size_t workspace_bytes, void* stream);
/* The same for a CHAIN (round 4): below_tables / below_zf / below_width -- the frequency-domain layer below, whose output gradient
 * dx is.  When the shapes allow (at most 8 blocks of 64 frames per utterance, batch x blocks a multiple of 128, at most 4 frames
 * of a block's window in either neighbour block) ONE launch inverts every block at its whole window, overlap-adds through LDS,
 * masks, stores dx and -- the frames still in registers -- writes the layer below's dz spectra to below_zf (*below_zf_written = 1:
 * skip st_conv1d_fft_dz_spectra_f32 for that layer).  below_* may be NULL / 0: the window-form inverse alone. */
int st_conv1d_nwc_bwd_data_fft_chain_f32(const st_tensor3* dz, const float* zf, const float* gfwd, int width, int pad_left,
                                         const st_tensor3* act, const st_tensor3* dx, const float* tables, const float* below_tables,
                                         float* below_zf, int below_width, int* below_zf_written, void* workspace,
                                         size_t workspace_bytes, void* stream);
int st_conv1d_nwc_bwd_filter_fft_f32(const st_tensor3* x, const st_tensor3* dz, const float* sf, const float* zf, int width,
                                     const float* tables, float* dpacked, void* workspace, size_t workspace_bytes,
                                     void* stream);

/* ---- the same three operations with the per-bin products on the bf16 matrix pipe (round 4) --------------------------------
 * planes = 1: BASELINE configs[3] arithmetic -- the tensors are read / written in their bf16 form (x_bf16, y_bf16, ...: same
 *             padded NWC geometry as the descriptor, 2-byte elements), spectra and filter spectra are one bf16 plane; the
 *             DFTs, the products' accumulation and the inverse DFTs are fp32.
 * planes = 3: fp32 tensors (the *_bf16 arguments NULL); every spectrum value is split exactly into three bf16 planes and a
 *             product taken as the six largest cross terms with fp32 accumulation: at least fp32-FMA accuracy at the bf16
 *             pipe's rate.
 * Buffers (elements of 2 bytes unless noted): sf_planes / zf_planes = planes x the fp32 form's float count
 * (st_conv1d_fft_sf_floats / _zf_floats); g_planes, gt_planes = planes x st_conv1d_fft_filter_plane_elems each (the filter
 * spectra and their per-bin transposes, rebuilt by st_conv1d_fft_filters_planes whenever the weights change); dc = fp32
 * [rows_pad][n_pad]: the blocks' frame sums (bin 0) kept in fp32 for the bias gradient (st_conv1d_fft_bias_grad_dc_f32 with
 * rows = batch x blocks); workspace st_conv1d_fft_planes_ws bytes. */
size_t st_conv1d_fft_filter_plane_elems(int width, int cin_pitch, int cout);
int st_conv1d_fft_filters_planes(const float* packed, int width, int cin, int cout, int cin_pitch, const float* tables, void* g_planes,
                                 void* gt_planes, int planes, void* stream);
size_t st_conv1d_fft_planes_ws(const st_tensor3* x, const st_tensor3* y, int width, int planes);
int st_conv1d_nwc_fwd_fft_planes(const st_tensor3* x, const void* x_bf16, const void* gt_planes, const float* bias, int width,
                                 int pad_left, int relu, const st_tensor3* y, void* y_bf16, const float* tables, void* sf_planes,
                                 int planes, void* workspace, size_t workspace_bytes, void* stream);
int st_conv1d_fft_dz_spectra_planes(const st_tensor3* dz, const void* dz_bf16, int width, const float* tables, void* zf_planes,
                                    int planes, float* dc, void* stream);
int st_conv1d_fft_bias_grad_dc_f32(const float* dc, int rows, int channels, int n_pad, float* dbias, void* stream);
int st_conv1d_nwc_bwd_data_fft_planes(const st_tensor3* dz, const void* zf_planes, const void* g_planes, int width, int pad_left,
                                      const st_tensor3* act, const void* act_bf16, const st_tensor3* dx, void* dx_bf16,
                                      const float* tables, int planes, void* workspace, size_t workspace_bytes, void* stream);
int st_conv1d_nwc_bwd_filter_fft_planes(const st_tensor3* x, const st_tensor3* dz, const void* sf_planes, const void* zf_planes, int width,
                                        const float* tables, float* dpacked, int planes, void* workspace, size_t workspace_bytes,
                                        void* stream);

/* ---- K11: back-prop (optimizer.compute_gradients, speech_model.py:78) -------------------
 * bwd_data: dx[b,t,c] = mask * sum_{w,o} dz[b, t + pad_left - w, o] * F[w,c,o]   (stride 1),
 *   mask = (act[b,t,c] > 0) when act != NULL (tf.nn.relu's gradient of the producing layer).
 *   packed_t comes from st_filters_flip_transpose_f32; dz->halo >= width-1-pad_left.  The workspace
 *   (st_conv1d_bwd_data_ws bytes, may be 0 / NULL) enables split-K for long reductions.
 * bwd_filter: dF[w,c,o] = sum_{b,t} x[b, t*stride + w - pad_left, c] * dz[b,t,o] in packed
 *   layout [k_pad][n_pad]; dbias[o] = sum_{b,t} dz[b,t,o].  Workspace: st_conv1d_bwd_filter_ws. */
size_t st_conv1d_bwd_data_ws(const st_tensor3* dz, const st_tensor3* dx, int width);
int st_conv1d_nwc_bwd_data_f32(const st_tensor3* dz, const float* packed_t, int width,
                               int pad_left, const st_tensor3* act, const st_tensor3* dx,
                               void* workspace, size_t workspace_bytes, void* stream);
/* Same, and additionally dbias_dx[n_pad of dx->channels] = column sums of the dx just written: the bias gradient
 * of the layer BELOW (its pre-activation gradient is dx), collected in the epilogue of the kernel that writes dx
 * instead of by a second pass over up to 129 MB.  Workspace: st_conv1d_bwd_data_bias_ws bytes. */
size_t st_conv1d_bwd_data_bias_ws(const st_tensor3* dz, const st_tensor3* dx, int width);
int st_conv1d_nwc_bwd_data_bias_f32(const st_tensor3* dz, const float* packed_t, int width, int pad_left,
                                    const st_tensor3* act, const st_tensor3* dx, float* dbias_dx,
                                    void* workspace, size_t workspace_bytes, void* stream);
/* The same for a ONE-TAP layer (speech_model.py:288,292: the two 1 x 1 layers on top) without any derived operand:
 * dx = dz W^T with `packed` the layer's own forward filters [cin_pitch][n_pad(cout)], read as a transposed operand.
 * Needs dz->c_pitch % 32 == 0 and an input width that packs to a multiple of 128; dbias_dx may be NULL.  Workspace as above
 * with width = 1. */
int st_conv1d_1tap_bwd_data_bias_f32(const st_tensor3* dz, const float* packed, const st_tensor3* act, const st_tensor3* dx,
                                     float* dbias_dx, void* workspace, size_t workspace_bytes, void* stream);
size_t st_conv1d_bwd_filter_ws(const st_tensor3* x, const st_tensor3* dz, int width);
/* bias gradient alone: dbias[o] = sum_{b,t} dz[b,t,o]  (n_pad floats) */
size_t st_bias_grad_ws(const st_tensor3* dz);
int st_bias_grad_f32(const st_tensor3* dz, float* dbias, void* workspace, size_t workspace_bytes, void* stream);
int st_conv1d_nwc_bwd_filter_f32(const st_tensor3* x, const st_tensor3* dz, int width, int stride,
                                 int pad_left, float* dpacked, float* dbias, void* workspace,
                                 size_t workspace_bytes, void* stream);

/* ---- K9-K10: tf.nn.ctc_loss + reduce_mean gradient (speech_model.py:74-75) --------------
 * logits: [B, T', C] padded NWC (halo 0), blank = C-1 (C <= 32).  labels CSR: label_offsets
 * [B+1], label_ids [label_offsets[B]].  seq_lens[b] = frames to use (reference passes
 * sequence_lengths // 2).  Outputs: loss[b] = -log p(l|x); grad = grad_scale * dloss/dlogits
 * (0 for t >= seq_lens[b]); status[b] != 0 when the label does not fit ("Not enough time for
 * target transition sequence": seq_lens[b] < L + adjacent repeats, seq_lens[b] outside 0..frames, L beyond what max_label_len
 * was dispatched for, or a negative L, i.e. label_offsets that do not increase) -- then loss = +inf and grad = 0.  A negative
 * max_label_len counts as 0.  The forward-backward lattice is kept as mantissa * 2^exponent
 * with an integer exponent per state (not in log space): exact range, no transcendental on the sequential chain; a class more than
 * 2^-30000 below its frame's best counts as impossible.  Workspace: st_ctc_ws bytes (log-softmax, emission factors, two lattices).
 * The two tensors may differ in halo, t_pitch and c_pitch (logits: c_pitch >= 32).  Of the logits only columns < C of frames
 * 0 .. frames-1 are read -- never a pitch column, a halo row or a row beyond the frames -- and what rows t >= seq_lens[b] hold
 * changes no output bit (the log-softmax does run over those rows, into scratch nobody reads).  Of grad,
 * columns 0 .. min(c_pitch, 32) - 1 of every frame 0 .. frames-1 are written: zeros in columns >= C, in rows t >= seq_lens[b]
 * and in every row of a refused utterance; columns >= 32, halo rows and rows beyond the frames are left untouched.  An empty
 * label over seq_lens[b] = 0 frames is valid: loss exactly 0.  Every utterance's result is independent of the rest of the
 * batch and the same bits from run to run. */
size_t st_ctc_ws(int batch, int frames, int max_label_len);
int st_ctc_loss_grad_f32(const st_tensor3* logits, const int32_t* label_ids,
                         const int32_t* label_offsets, const int32_t* seq_lens, int max_label_len,
                         float grad_scale, float* loss, const st_tensor3* grad, int32_t* status,
                         void* workspace, size_t workspace_bytes, void* stream);
/* The same with the loss as a (hi, lo) float pair: loss[b] is the fp32 value above (what TF's fp32 op returns), loss_lo[b]
 * (may be null) the part of -log p that fp32 cannot hold at that magnitude -- the kernel knows log p in double (the lattice
 * rounds 6e-8 relative per step, one fp32 ulp of a loss of 1 239 is 1.2e-4); (double)loss[b] + loss_lo[b] is the loss to
 * ~1e-6 of the float64 oracle.  speech_model.py:74-75: avg_loss = mean of these. */
int st_ctc_loss_grad_hilo_f32(const st_tensor3* logits, const int32_t* label_ids,
                              const int32_t* label_offsets, const int32_t* seq_lens, int max_label_len,
                              float grad_scale, float* loss, float* loss_lo, const st_tensor3* grad, int32_t* status,
                              void* workspace, size_t workspace_bytes, void* stream);
/* The same for partial transcripts: label ids may hold the wildcard, id num_classes (the slot after the blank, as in
 * st_ctc_align_wild_f32), so num_classes <= 31 here.  The wildcard is a label state of the 2L+1 lattice like any other (blanks
 * around it, at least one frame, the same skip rules, never two in a row; it counts as a label towards "not enough frames")
 * whose emission is  w_t = e^wildcard_bias * sum_{c < blank} y_t(c),  wildcard_bias <= 0 in nats per frame: the frame reads
 * some label, at a price (the star of Star Temporal Classification, Pratap et al. 2022, without its minus-next-token term).
 * loss = -ln sum_paths prod emissions; grad[b,t,k] = grad_scale * (y_t(k) - occ_t(k) - [k < blank] occ_t(wild) y_t(k) / S_t),
 * S_t = sum_{c < blank} y_t(c); the wildcard is no logit, columns num_classes .. 31 stay zero.  An utterance without a wildcard
 * gets the bits of st_ctc_loss_grad_hilo_f32 (loss, loss_lo, status, gradient), whatever else the batch holds.  The gradient's
 * wildcard term recovers log2 S_t from the fp32 value log2 S_t + wildcard_bias * log2 e that the workspace rows hold: its relative
 * error grows with |wildcard_bias| (about 1e-7 per nat; negligible at a price of a few nats per frame, 1e-5 at hundreds).  Workspace:
 * st_ctc_ws.  (tests/wild_ctc_oracle.py is the specification.) */
int st_ctc_loss_grad_wild_f32(const st_tensor3* logits, const int32_t* label_ids,
                              const int32_t* label_offsets, const int32_t* seq_lens, int max_label_len,
                              float grad_scale, double wildcard_bias, float* loss, float* loss_lo, const st_tensor3* grad,
                              int32_t* status, void* workspace, size_t workspace_bytes, void* stream);

/* ---- K14: tf.nn.ctc_greedy_decoder(merge_repeated) (speech_model.py:113-115) ------------
 * ids [B][max_out] int32 (max_out >= frames), out_lens [B], neg_sum_logits [B].  Row b of ids is written in its first
 * out_lens[b] entries only, the rest is left untouched.  With a max_out smaller than an utterance's output, out_lens[b] still
 * is the full count and the first max_out ids are written.  Logits are read in columns < C of frames t < seq_lens[b] alone. */
int st_ctc_greedy_decode(const st_tensor3* logits, const int32_t* seq_lens, int merge_repeated,
                         int32_t* ids, int max_out, int32_t* out_lens, float* neg_sum_logits,
                         void* stream);

/* ---- Forced alignment: the best-path (Viterbi) CTC alignment of given labels (csrc/ctc_align.hip) ----
 * Conventions of st_ctc_loss_grad_f32: logits [B, T', C] padded NWC, blank = C-1, C <= 32, labels CSR, labels up to 511
 * (max_label_len picks the same states-per-lane dispatch), enqueues only, never allocates.
 *
 * Semantics (the float64 specification is tests/align_oracle.py).  The lattice of utterance b has U = 2L+1 states: even
 * states are blanks, odd state u is label (u-1)/2.  A path assigns one state to each of the seq_lens[b] frames; it
 *  - starts in state 0 or 1 and ends in state U-1 or U-2,
 *  - moves by 0 (stay), 1 (advance) or 2 (skip) states per frame, the skip only from a label to a DIFFERENT label,
 *  - and the one returned maximises sum_t ln softmax(logits[t])[class of the state at t].
 * Ties go to the smaller move: stay, then advance, then skip (decided at the later frame, over the best scores of the three
 * predecessors); a tie at the end goes to the last label state.  L = 0 is valid: every frame is blank, spans is empty.
 * Logits may be -inf for single classes; if that leaves no path of finite score, score = -inf and spans / states are
 * unspecified (status stays 0).
 *
 * Outputs: spans [label_offsets[B]][2] = first frame, one past the last frame spent in that label's state;
 * states [B][frames] (may be null) = label index at each frame, -1 = blank, -2 = frame >= seq_lens[b];
 * score [B] = ln p(best path), rounded to float from the double the lattice is kept in;
 * status [B] != 0: the label does not fit (seq_lens[b] < L + adjacent repeats, seq_lens[b] outside 0..frames, L beyond
 * what max_label_len was dispatched for, or a negative L: the rule of st_ctc_loss_grad_f32, csrc/ctc_lattice.h) -- then score = -inf, the utterance's spans are {-1, -1} and all its states -2.
 * Every output is written with ordinary vector stores.
 *
 * Workspace (16-byte aligned): st_ctc_align_ws = batch * frames * (32 * 8 + 64 * 4) + batch * 4 + 512 bytes for
 * 0 <= max_label_len <= 511 and batch, frames > 0 (else 0): the ln-softmax rows in double, one 256-byte back-pointer row per
 * frame (2 bits per state, one uint32 per lane) and the end states.
 *
 * st_ctc_align_host: the same recursion (shared arithmetic, csrc/ctc_align_core.h: identical paths, ties included) on HOST
 * pointers, logits as a dense [batch][frames][classes] array; needs no device. */
size_t st_ctc_align_ws(int batch, int frames, int max_label_len);
int st_ctc_align_f32(const st_tensor3* logits, const int32_t* label_ids, const int32_t* label_offsets,
                     const int32_t* seq_lens, int max_label_len, int32_t* spans, int32_t* states, float* score,
                     int32_t* status, void* workspace, size_t workspace_bytes, void* stream);
int st_ctc_align_host(const float* logits, int batch, int frames, int classes, const int32_t* label_ids,
                      const int32_t* label_offsets, const int32_t* seq_lens, int max_label_len, int32_t* spans,
                      int32_t* states, float* score, int32_t* status, void* workspace, size_t workspace_bytes);

/* ---- Forced alignment of one long sequence: the same lattice in tiles (csrc/ctc_align_long.hip) ----
 * The semantics of st_ctc_align_f32 -- lattice, moves, tie rules, end rule, fit rule -- for ONE sequence whose label may
 * hold up to 1 048 575 ids: a transcript against the concatenated output frames of a long recording.  On a label that
 * st_ctc_align_f32 takes, both return the same spans and the same score (there rounded to float).
 *
 * logits: dense [frames][row_pitch] floats, columns < classes are read; 2 <= classes <= 32, classes <= row_pitch,
 * blank = classes - 1; 0 < frames <= 2^31 - 65.  label_ids [label_len], ids in [0, classes - 1): the kernel indexes rows with
 * them and does not check.  label_len = 0 is valid (label_ids may then be null).  On the device entry logits, label_ids and all
 * outputs are device pointers; it enqueues only and never allocates.
 *
 * Outputs: spans [label_len][2] as st_ctc_align_f32 writes them; score [1] = ln p(best path) as the DOUBLE the lattice is
 * kept in; status [1] != 0: the label does not fit (frames < label_len + adjacent repeats) -- then score = -inf and the spans
 * are {-1, -1}.  There is no `states` output.  Every output and workspace write is an ordinary vector store.
 *
 * How it runs: a frame block is 64 frames, a state block the 896 states one wave owns (16 per lane in lanes 8-63; lanes 0-7
 * recompute a halo of 128 states from the neighbouring block's column, which is exact because a state looks at most two
 * states down per frame).  2 + ceil(frames / 64) + 1 stream-ordered launches: log-softmax rows, init, one launch of
 * NB = ceil((2 label_len + 1) / 896) workgroups per frame block, one back-trace wave.  The launch boundary is the only
 * synchronisation between workgroups.
 *
 * Workspace (16-byte aligned): st_ctc_align_long_ws = frames * (32 * 8 + 56 * 4 * NB) + 2 * (896 * NB + 128) * 8 + 512 bytes
 * for frames > 0 and 0 <= label_len <= 1 048 575 (else 0): the ln-softmax rows in double, the back-pointer rows (2 bits per
 * state, 56 uint32 per state block and frame) and two lattice columns.  The call defines all of it that it reads.
 *
 * st_ctc_align_long_host: plain loops over the whole lattice with the same arithmetic (csrc/ctc_align_core.h) and the same
 * back-pointer layout on HOST pointers: identical spans, score bits and status; needs no device. */
size_t st_ctc_align_long_ws(long frames, int label_len);
int st_ctc_align_long_f32(const float* logits, long frames, int classes, int row_pitch, const int32_t* label_ids, int label_len,
                          int32_t* spans, double* score, int32_t* status, void* workspace, size_t workspace_bytes,
                          void* stream);
int st_ctc_align_long_host(const float* logits, long frames, int classes, int row_pitch, const int32_t* label_ids, int label_len,
                           int32_t* spans, double* score, int32_t* status, void* workspace, size_t workspace_bytes);

/* ---- Forced alignment of transcripts that leave audio out: a wildcard label and a per-label fit ----
 * st_ctc_align_wild_f32 and st_ctc_align_long_wild_f32 are st_ctc_align_f32 and st_ctc_align_long_f32 -- the same lattice and
 * back-trace kernels, ties, end rule, fit rule, score, spans, workspace sizes (st_ctc_align_ws, st_ctc_align_long_ws) -- with two
 * additions.  The float64 specification is tests/wildcard_align_oracle.py.
 *
 * The wildcard W is the id `classes`, one past the blank; ids are therefore in [0, classes - 1) or == classes, and
 * 2 <= classes <= 31 (ST_EINVAL above): the ln-softmax rows are [32] wide and slot `classes`, -inf in the plain entry points,
 * holds W's emission.  W is a label state like any other: it takes at least one frame, counts as one label in the fit rule
 * frames >= L + adjacent repeats, and its class differs from every id, so the skip over the blank into it and out of it is
 * allowed.  Its emission at frame t is the largest of the row's `classes` ln-softmax values, the blank included, plus
 * wildcard_bias, in double: ly_t(W) = max_c ly_t(c) + wildcard_bias.  wildcard_bias is finite and <= 0 (ST_EINVAL otherwise).
 * With a bias of 0 the wildcard ties with a label on every frame the greedy reading agrees with, and the tie rule hands such
 * frames to the wildcard that follows; a negative bias is the price per frame of not reading the transcript.  The span of a
 * wildcard is the stretch of audio the transcript leaves out.  Two ADJACENT wildcards are a bad argument: the host forms
 * return ST_EINVAL; the device forms cannot read the labels where they validate, and, as for the range of the ids, the caller
 * checks (engine.align does).  Without a wildcard among the labels the spans, states, score bits and status are those of the
 * plain entry points, whatever the bias.
 *
 * fit (may be null; [label_offsets[B]] resp. [label_len] doubles): the best path gives label k of class c_k the frames [a, b);
 * fit_k = sum over t = a .. b-1, in frame order, of ly_t(c_k) - max_c ly_t(c), in double: exactly 0 where the greedy reading
 * spells the label on every one of its frames, negative otherwise.  For a wildcard fit_k = wildcard_bias * (b - a), one
 * product.  Blank frames belong to no label.  The labels of an utterance with status != 0 get NaN.  The fit stage runs after
 * the back-trace, on the rows still in the workspace: one pass turns slot `classes` of every row into the row's maximum, then
 * one lane per label walks its span (a label forced over thousands of frames is a serial walk of that length).  With
 * fit = null the stage is not launched.
 *
 * The host forms share the deciding arithmetic (csrc/ctc_align_core.h): identical spans, states, score bits, status and fit
 * bits; they also check every id against 0 .. classes. */
int st_ctc_align_wild_f32(const st_tensor3* logits, const int32_t* label_ids, const int32_t* label_offsets,
                          const int32_t* seq_lens, int max_label_len, double wildcard_bias, int32_t* spans, int32_t* states,
                          float* score, int32_t* status, double* fit, void* workspace, size_t workspace_bytes, void* stream);
int st_ctc_align_wild_host(const float* logits, int batch, int frames, int classes, const int32_t* label_ids,
                           const int32_t* label_offsets, const int32_t* seq_lens, int max_label_len, double wildcard_bias,
                           int32_t* spans, int32_t* states, float* score, int32_t* status, double* fit, void* workspace,
                           size_t workspace_bytes);
int st_ctc_align_long_wild_f32(const float* logits, long frames, int classes, int row_pitch, const int32_t* label_ids, int label_len,
                               double wildcard_bias, int32_t* spans, double* score, int32_t* status, double* fit, void* workspace,
                               size_t workspace_bytes, void* stream);
int st_ctc_align_long_wild_host(const float* logits, long frames, int classes, int row_pitch, const int32_t* label_ids, int label_len,
                                double wildcard_bias, int32_t* spans, double* score, int32_t* status, double* fit, void* workspace,
                                size_t workspace_bytes);

/* ---- Word confidences: exact CTC word posteriors of given labels (csrc/ctc_conf.hip) ----
 * Conventions of st_ctc_align_f32: logits [B, T', C] padded NWC, blank = C-1, labels CSR, labels up to 511 (max_label_len
 * picks the states-per-lane dispatch), seq_lens[b] frames are used, enqueues only, never allocates.  Here C <= 30 (two
 * columns of the 32-wide softmax row carry the pseudo-label and the dead blanks; ST_EINVAL above that) and
 * 0 <= space_id < C-1 is the id that separates words.
 *
 * Semantics (the float64 specification is tests/conf_oracle.py), with p_t(c) = softmax(logits[t])[c]:
 *  - the words of a label l are its maximal runs of ids other than space_id;
 *  - P(l) is the CTC probability of l, the sum over all alignments (exp(-loss) of st_ctc_loss_grad_f32);
 *  - P(l*j): the ids of word j are replaced by ONE pseudo-label * and the standard lattice (2L'+1 states, blanks between
 *    labels, a skip only between different labels) is run with two changes: the * state emits sum_{c != space_id} p_t(c),
 *    the blank included, and the two blank states beside * are impossible (emission 0).  * differs from both neighbours.
 *    Every alignment of l is counted once in the * path with the same word boundaries: 0 < P(l) <= P(l*j).
 *  - log_prob[b] = ln P(l); log_conf[w] = min(0, ln P(l) - ln P(l*j)): the log of the probability that the stretch between
 *    the word's neighbouring spaces reads that word, given that all other words read as in l, word boundaries summed out.
 *    P(l) = 0 (single -inf logits can do that): log_prob = -inf and log_conf = -inf.
 *  - status [B] != 0: the label is refused by the rule of st_ctc_loss_grad_f32 and st_ctc_align_f32 (csrc/ctc_lattice.h);
 *    then log_prob = -inf and the log_conf of that utterance's words are NaN.  L = 0 is valid: log_prob = sum_t ln p_t(blank).
 *
 * word_spans: DEVICE [n_words][3] = utterance, first label index, one past the last, made by the host from the ids; the
 * words of all utterances in any order, log_conf [n_words] in the same order.  A span that is not a maximal non-space run of
 * its utterance is the caller's error: the result is unspecified, but nothing outside the outputs is written and nothing
 * outside the inputs is read (a span outside its label, or an utterance outside the batch, gives NaN).  The same holds for
 * ids outside 0 .. C-2.  n_words = 0 is valid (word_spans and log_conf may then be null).
 *
 * Arithmetic: sum-product in the linear domain, IEEE double, a state's value kept as mantissa * 2^exponent with an integer
 * exponent per state (rescaling moves exponent bits: exact); no transcendental on the frame chain.  Every output is written
 * with ordinary vector stores.
 *
 * Workspace (16-byte aligned): st_ctc_word_conf_ws = batch * frames * 32 * 8 + max_jobs * 8 + 512 bytes for
 * 0 <= max_label_len <= 511, batch, frames > 0 and max_jobs >= batch + n_words (else 0): the softmax rows in double, written
 * once per utterance, and ln P of every job -- one full label per utterance and one * lattice per word, one wave each.
 *
 * st_ctc_word_conf_host: the same recursion (shared arithmetic, csrc/ctc_conf_core.h: the same BITS) on HOST pointers,
 * word_spans included, logits as a dense [batch][frames][classes] array; needs no device. */
size_t st_ctc_word_conf_ws(int batch, int frames, int max_label_len, int max_jobs);
int st_ctc_word_conf_f32(const st_tensor3* logits, const int32_t* label_ids, const int32_t* label_offsets,
                         const int32_t* seq_lens, int max_label_len, int space_id, const int32_t* word_spans, int n_words,
                         double* log_prob, double* log_conf, int32_t* status, void* workspace, size_t workspace_bytes,
                         void* stream);
int st_ctc_word_conf_host(const float* logits, int batch, int frames, int classes, const int32_t* label_ids,
                          const int32_t* label_offsets, const int32_t* seq_lens, int max_label_len, int space_id,
                          const int32_t* word_spans, int n_words, double* log_prob, double* log_conf, int32_t* status,
                          void* workspace, size_t workspace_bytes);

/* ---- Keyword spotting: the best occurrence of given keywords in given utterances (csrc/ctc_spot.hip) ----
 * Conventions of st_ctc_align_f32 / st_ctc_word_conf_f32: logits [B, T', C] padded NWC, blank = C-1, C <= 32, seq_lens[b]
 * frames are used, only columns < C of frames < seq_lens[b] influence any output bit (a pitch column, a halo row or a row beyond
 * `frames` is never read), enqueues only, never allocates.  Keywords are CSR: kw_ids, kw_offsets [n_keywords + 1], ids in
 * 0 .. C-2 (spaces allowed: a phrase), 1 <= L <= 511; max_keyword_len picks the states-per-lane dispatch.
 *
 * Semantics (the float64 specification is tests/spot_oracle.py).  Per frame m_t = max_c x_t(c) and
 * d_t(c) = (double)x_t(c) - (double)m_t: one IEEE double subtraction, <= 0, exactly 0 for the greedy class; it is the log of
 * the ratio of the class's softmax probability to the greedy class's -- the normaliser cancels, there is no exp or log.
 * An OCCURRENCE of keyword k over frames [s, e) is a frame path that is a CTC alignment of k, beginning on k_0 and ending on
 * k_{L-1} (no leading or trailing blank; blanks optional between labels, compulsory between equal neighbours; repeats
 * collapse); its score is sum_{t in [s,e)} d_t(class at t), the log-likelihood ratio of reading the keyword there against the
 * greedy reading of the same frames.  The spot score of (utterance, keyword) is the maximum over all s < e <= seq_lens[b] and
 * all such paths: <= 0, and == 0 exactly when the frame-wise argmax classes spell the keyword tightly somewhere.
 *
 * Recursion over t = 0 .. seq_lens[b]-1 on the 2L+1 CTC states; states 0 and 2L are dead (-inf).  Each state u = 1 .. 2L-1
 * carries a value v and a start frame s, v_{-1} = -inf, s_{-1} = -1:
 *   v_t(u) = best + d_t(class(u)), best over -- in this order, replaced only by a STRICTLY larger value --
 *     stay v_{t-1}(u), advance v_{t-1}(u-1), skip v_{t-1}(u-2) (a label that differs from the previous label), and for u = 1
 *     enter = 0.0 with start t;
 *   s_t(u) = the start of the predecessor taken (t for enter; -1 when best is -inf);  end_t = v_t(2L-1), start s_t(2L-1).
 * The result is the largest finite end_t, the LATEST t among equals (the frames on which the last character stays the argmax
 * add exact zeros and belong to the hit): score = end_t, span = {s_t(2L-1), t+1}.  No finite end_t (a keyword that needs more
 * frames than the utterance has): score = -inf, span = {-1, -1}, status = 0.
 *
 * jobs: DEVICE [n_jobs][2] = utterance, keyword, in any order, repeats allowed; one wave each.  Outputs per job: score
 * (double), span [2], status; and, when both trace pointers are given, trace_score [n_jobs][frames] = end_t and trace_start
 * [n_jobs][frames] = s_t(2L-1), -inf and -1 for t >= seq_lens[b].  status != 0: the utterance or the keyword index lies outside
 * its table, L < 1 or beyond what max_keyword_len was dispatched for, kw_offsets not monotone there, or seq_lens[b] outside
 * 0 .. frames -- then score = -inf, span = {-1, -1} and the job's trace rows are -inf / -1 throughout.  A row whose largest
 * logit is not finite makes that job's result unspecified (single -inf logits are fine); ids outside 0 .. C-2 likewise; even
 * then nothing outside the outputs is written and nothing outside the inputs is read.  n_jobs = 0 is valid.  Every output is
 * written with ordinary vector stores.
 *
 * Workspace (16-byte aligned): st_ctc_spot_ws = batch * frames * 32 * 8 + 512 bytes for 1 <= max_keyword_len <= 511, batch,
 * frames > 0 and n_jobs >= 0 (else 0): the rows of d in double, written once per utterance.  The start travels with the
 * value: no back-pointer rows, no back-trace, nothing that grows with n_jobs * frames.
 *
 * st_ctc_spot_host: the same recursion (shared arithmetic, csrc/ctc_spot_core.h: the same BITS) on HOST pointers, jobs
 * included, logits as a dense [batch][frames][classes] array; needs no device. */
size_t st_ctc_spot_ws(int batch, int frames, int max_keyword_len, int n_jobs);
int st_ctc_spot_f32(const st_tensor3* logits, const int32_t* seq_lens, const int32_t* kw_ids, const int32_t* kw_offsets,
                    int n_keywords, int max_keyword_len, const int32_t* jobs, int n_jobs, double* score, int32_t* span,
                    double* trace_score, int32_t* trace_start, int32_t* status, void* workspace, size_t workspace_bytes,
                    void* stream);
int st_ctc_spot_host(const float* logits, int batch, int frames, int classes, const int32_t* seq_lens, const int32_t* kw_ids,
                     const int32_t* kw_offsets, int n_keywords, int max_keyword_len, const int32_t* jobs, int n_jobs,
                     double* score, int32_t* span, double* trace_score, int32_t* trace_start, int32_t* status, void* workspace,
                     size_t workspace_bytes);

/* ---- LM-free CTC prefix beam search, top path (BASELINE config 5) -----
 * The reference only reaches a beam search through its KenLM TensorFlow fork
 * (speech_model.py:101-111: beam_width=100, merge_repeated=False, top_paths=1); this is the stock
 * tf.nn.ctc_beam_search_decoder recursion without a scorer.  blank = C-1, C <= 32, beam <= 128 (one wavefront per
 * utterance; beams above 64 run a two-entries-per-lane instantiation with an exact W-th-largest selection bound).
 * ids [B][max_out] int32 (labels beyond max_out are dropped, out_lens still reports the true
 * length), log_prob [B] = ln p(top prefix) under the per-frame softmax.  The labels are the top prefix itself, i.e.
 * merge_repeated=False as the reference asks (speech_model.py:110); collapsing repeats is a host-side option. */
size_t st_ctc_beam_ws(int batch, int frames, int beam_width);
int st_ctc_beam_search_decode(const st_tensor3* logits, const int32_t* seq_lens, int beam_width,
                              int32_t* ids, int max_out, int32_t* out_lens, float* log_prob,
                              void* workspace, size_t workspace_bytes, void* stream);
/* ... with the reference's input transform: input_transform = 1 searches on log10(softmax(logits) + 1e-8), what
 * speech_model.py:102 hands the decoder (which normalises it per frame like any input); 0 = the logits themselves. */
int st_ctc_beam_search_decode_ex(const st_tensor3* logits, const int32_t* seq_lens, int beam_width, int input_transform,
                                 int32_t* ids, int max_out, int32_t* out_lens, float* log_prob,
                                 void* workspace, size_t workspace_bytes, void* stream);

/* ---- word n-gram language model + LM-scored CTC prefix beam search (the reference's KenLM decoder path,
 * speech_model.py:84-111; semantics restated in tests/lm_oracle.py) ---------------------------------------------------
 * st_lm_create_arpa parses an ARPA model (orders 1..5) from a memory buffer into host tables: word ids (<unk> 0, <s> 1,
 * </s> 2, then the unigrams in file order, lowercased), one open-addressing hash per order holding float32 log10 p and
 * backoff, and a character trie over the words spelled in [a-z'] (other words keep their n-grams, unreachable from the
 * trie: `skipped_words`).  A format error returns ST_EINVAL with "ARPA line N: ..." in err (and st_last_error).
 * st_lm_upload copies the tables to the device of `stream` (null: the current device), once per device and handle; the
 * decoder uses the copy on its own stream's device and refuses a handle without one.  st_lm_query_host / st_lm_trie_lookup /
 * st_lm_word_id read the host tables (the same lookup code the kernel runs). */
int st_lm_create_arpa(const char* text, size_t bytes, void** handle, char* err, size_t errlen);
/* counts: order + 1 entries: counts[0] = word ids (with <unk> <s> </s>), counts[n] = n-grams of order n */
int st_lm_info(void* handle, int* order, int64_t* counts, int64_t* skipped_words, int64_t* trie_nodes, size_t* device_bytes);
int st_lm_upload(void* handle, void* stream);
int st_lm_word_id(void* handle, const char* word, int32_t* id);            /* <unk> (0) for a word not in the model */
/* log10 p(word | ctx[0..n-1]) with ARPA backoff (the last order - 1 context words are used) */
int st_lm_query_host(void* handle, const int32_t* ctx, int n, int32_t word, float* logp);
int st_lm_trie_lookup(void* handle, const char* prefix, int32_t* node, float* min_logp, int32_t* word);
int st_lm_destroy(void* handle);
/* The prefix beam search of st_ctc_beam_search_decode_ex with TF's scorer hooks: a word n-gram score enters every transition
 * into a prefix as lm_weight * (its LM score - its parent's); a word is scored when a space follows it (+ word_count_weight, +
 * valid_word_count_weight if in the vocabulary), an incomplete word by the lowest unigram of its completions (oov_score once
 * it has left the vocabulary); at the end of the utterance every entry scores its incomplete word and </s>, and the top path
 * is the best total after that.  Classes: a-z ' space blank (C = 29); beam <= 128; workspace: st_ctc_beam_ws; `lm` uploaded to
 * the device of `stream`.
 * log_prob includes the LM terms. */
int st_ctc_beam_search_decode_lm(const st_tensor3* logits, const int32_t* seq_lens, int beam_width, int input_transform, void* lm,
                                 float lm_weight, float word_count_weight, float valid_word_count_weight, float oov_score,
                                 int32_t* ids, int max_out, int32_t* out_lens, float* log_prob, void* workspace,
                                 size_t workspace_bytes, void* stream);
/* The same search for several weight triples at once (the LM weight search scores a generation of candidates on one batch): the
 * log-softmax rows are computed once, and one launch of (batch x candidates) blocks decodes every (candidate, utterance) pair
 * with its own node pool.  weights: HOST [candidates][3] = {lm_weight, word_count_weight, valid_word_count_weight}, all finite;
 * candidates >= 1.  A launch takes at most 64 triples (kernel-argument space); more are split into launches of 64 that reuse the
 * same node pools in stream order, so the workspace (st_ctc_beam_lm_candidates_ws) grows with min(candidates, 64).  Outputs per
 * candidate p: ids [p][batch][max_out], out_lens [p][batch], log_prob [p][batch], each bit-identical to
 * st_ctc_beam_search_decode_lm with p's weights (which is this entry point with one triple). */
size_t st_ctc_beam_lm_candidates_ws(int batch, int frames, int beam_width, int candidates);
int st_ctc_beam_search_decode_lm_candidates(const st_tensor3* logits, const int32_t* seq_lens, int beam_width, int input_transform,
                                            void* lm, const float* weights, int candidates, float oov_score, int32_t* ids,
                                            int max_out, int32_t* out_lens, float* log_prob, void* workspace,
                                            size_t workspace_bytes, void* stream);

/* ---- N-best lists from both beam searches ------------------------------------------------------------------------------
 * The same searches (the frame loop is the same code), returning the n_best best final entries instead of the top path;
 * 1 <= n_best <= beam_width; workspace: st_ctc_beam_ws.  Outputs: ids [B][n_best][max_out], out_lens [B][n_best], log_prob
 * [B][n_best] float32, n_hyps [B].  Ranking (restated in tests/nbest_oracle.py):
 *   - LM-free: the hypotheses are entries 0 .. n-1 of the final beam set, which is sorted by (total desc, candidate key asc);
 *   - LM: every entry first gains its end-of-utterance delta (incomplete word, then </s>), exactly as for the top path; the
 *     entries are then ranked by (final total desc, rank in the set asc);
 *   - n_hyps[b] = min(n_best, entries alive): an utterance of length 0 has one entry, the empty prefix;
 *   - slots at or beyond n_hyps[b] get out_lens = 0 and log_prob = -inf;
 *   - labels beyond max_out are dropped and out_lens reports the true length;
 *   - merge_repeated=False: the host's collapsing option is not offered for lists (it could make two hypotheses equal).
 * n_best = 1 returns the bits of st_ctc_beam_search_decode_ex / st_ctc_beam_search_decode_lm. */
int st_ctc_beam_search_decode_nbest(const st_tensor3* logits, const int32_t* seq_lens, int beam_width, int input_transform, int n_best,
                                    int32_t* ids, int max_out, int32_t* out_lens, float* log_prob, int32_t* n_hyps, void* workspace,
                                    size_t workspace_bytes, void* stream);
int st_ctc_beam_search_decode_lm_nbest(const st_tensor3* logits, const int32_t* seq_lens, int beam_width, int input_transform, void* lm,
                                       float lm_weight, float word_count_weight, float valid_word_count_weight, float oov_score,
                                       int n_best, int32_t* ids, int max_out, int32_t* out_lens, float* log_prob, int32_t* n_hyps,
                                       void* workspace, size_t workspace_bytes, void* stream);

/* ---- hotword biasing of both beam searches -----------------------------------------------------------------------------
 * K phrases of 1..64 ids in 0..27 and one weight w >= 0 per matched character: a hypothesis with prefix x scores, during the search,
 *   total(x) = CTC mass + lm_weight * LM terms (with a model) + w * (M(x) + r(x)),
 * M = the characters of completed phrase occurrences banked so far, r = the length of the partial match still open (a partial match
 * earns credit while it grows and gives it back when it fails); at the end of the utterance w * r(x) is replaced by what the flush
 * banks.  x is scanned left to right with a state n, a node of the phrases' trie whose path is the open match (the specification,
 * on strings: tests/hotword_oracle.py):
 *   - label c, (a): n has a child c: move to it; if that child ends a phrase and has no children, bank its depth, return to the root;
 *   - label c, (b) otherwise: at the root, stay.  Else let t be the deepest phrase-ending node on n's path (n included): bank
 *     depth(t) (0 without one), take u = the path without its first depth(t) characters (without its first character if there is
 *     no t), restart at the root and feed u, then c, by these same rules;
 *   - end of utterance (flush): repeat the resolution of (b) without a label until the state is the root; what is banked on the
 *     way counts, the rest is forfeited.
 * The rules are functions of (n, c) and of n, so the caller tabulates them (speecht_amd/hotwords.py) and the kernels read tables:
 *   next [n_states][32] int32, gain [n_states][32] float32 = w * (banked + depth(next) - depth(n)), fin [n_states] float32 =
 *   w * (flush bank - depth(n)); state 0 is the root; columns >= 28 hold the state itself and 0 (a label outside 0..27, which an
 *   LM-free search of more classes may have, neither advances nor breaks a match).  All three are DEVICE pointers on the device of
 *   `stream`, read while the search runs; 1 <= n_states <= 2^20.
 * The state is a function of the prefix alone, so merging prefixes by hash stays correct.  The gain enters wherever the LM's delta
 * does (child candidates, the stay candidate's parent inflow) and fin with the LM's end-of-utterance delta; BOTH searches then rank
 * the final set by (final total desc, rank in the set asc).  Everything else -- arguments, checks, workspace (st_ctc_beam_ws),
 * outputs -- is that of st_ctc_beam_search_decode_nbest / _lm_nbest; the top path of a biased search is its n_best = 1 list.  Tables
 * of one state, or whose gain and fin are all zero, return the bits of the unbiased entry points.  Every state read from `next` is
 * clamped to [0, n_states): a malformed table gives wrong text, never a read outside the tables. */
typedef struct st_bias_tables {
  const int32_t* next;
  const float* gain;
  const float* fin;
  int32_t n_states;
} st_bias_tables;
int st_ctc_beam_search_decode_bias_nbest(const st_tensor3* logits, const int32_t* seq_lens, int beam_width, int input_transform,
                                         const st_bias_tables* bias, int n_best, int32_t* ids, int max_out, int32_t* out_lens,
                                         float* log_prob, int32_t* n_hyps, void* workspace, size_t workspace_bytes, void* stream);
int st_ctc_beam_search_decode_lm_bias_nbest(const st_tensor3* logits, const int32_t* seq_lens, int beam_width, int input_transform,
                                            void* lm, float lm_weight, float word_count_weight, float valid_word_count_weight,
                                            float oov_score, const st_bias_tables* bias, int n_best, int32_t* ids, int max_out,
                                            int32_t* out_lens, float* log_prob, int32_t* n_hyps, void* workspace,
                                            size_t workspace_bytes, void* stream);

/* Sentence scores of n label prefixes (ids [n][pitch], lens [n], ids 0..27 = a-z ' space) under a model: what the LM search adds
 * to a final entry, without its weights -- a final total splits exactly as
 *   total = A + lm_weight * (G + word_count_weight * n_words + valid_word_count_weight * n_valid),  A = the acoustic mass;
 * oov_score never enters.  The ids are cut at every space into words; an empty run (a leading space, two spaces in a row) counts
 * as a word and scores as <unk>; the trailing run counts only if non-empty.  The context starts as <s> (order > 1) and keeps
 * the last order - 1 words.  A word spelled in [a-z'] that is a unigram scores as itself and counts in n_valid, any other as
 * <unk>.  g = sum of log10 p(word | ctx) + log10 p(</s> | ctx): float32 table values summed in double in word order, </s> last.
 * n = 0 is valid.  _f64: device pointers, `lm` uploaded to the device of `stream`; _host: host pointers, no device.  The two run
 * the same arithmetic (csrc/lm_score_core.h) and are bit-identical.  An id outside 0..27 or a length outside 0..pitch: the host
 * form returns ST_EINVAL and writes nothing; the device form, which cannot report without waiting for the stream, marks that
 * prefix with g = NaN and n_words = n_valid = -1. */
int st_lm_score_prefixes_f64(void* lm, const int32_t* ids, int pitch, const int32_t* lens, int n, double* g, int32_t* n_words,
                             int32_t* n_valid, void* stream);
int st_lm_score_prefixes_host(void* lm, const int32_t* ids, int pitch, const int32_t* lens, int n, double* g, int32_t* n_words,
                              int32_t* n_valid);

/* ---- exact Levenshtein distances of id sequences (the evaluation's letter and word edit distances, evaluation.py:40-49) ------
 * expected [expected_rows][expected_pitch] with lengths expected_lens, decoded [decoded_rows][decoded_pitch] with decoded_lens, all
 * device int32; pairs: DEVICE [n_pairs][2] = (expected row, decoded row).  distances: DEVICE [n_pairs][2] = {letter distance, word
 * distance}, where letters are the ids and words are the maximal runs of ids other than space (27): editdistance.eval of
 * ids_to_sentence and of its str.split() for ids 0..27.  A pair with an id outside 0..27, a length outside 0..min(pitch,
 * st_edit_distance_max_len()) or a row index out of range gets {-1, -1}: score it on the host.  No workspace. */
int st_edit_distance_max_len(void);
int st_edit_distance_pairs(const int32_t* expected, int expected_rows, int expected_pitch, const int32_t* expected_lens,
                           const int32_t* decoded, int decoded_rows, int decoded_pitch, const int32_t* decoded_lens,
                           const int32_t* pairs, int n_pairs, int32_t* distances, void* stream);

/* ---- K12-K13: clip_by_global_norm + AdamOptimizer(epsilon outside) (speech_model.py:77-82)
 * Flat fp32 buffers of n floats.  stats (device, 2 floats) receives {global_norm, scale}.
 * lr_t = lr * sqrt(1-beta2^t)/(1-beta1^t) is computed by the caller (host, double).
 * p -= lr_t * m / (sqrt(v) + eps) after m,v updates with g * scale. */
size_t st_global_norm_ws(size_t n);
int st_global_norm_clip_adam_f32(float* params, const float* grads, float* m, float* v, size_t n,
                                 float clip_norm, float lr_t, float beta1, float beta2, float eps,
                                 float* stats, void* workspace, size_t workspace_bytes,
                                 void* stream);
/* Gated form.  tf.nn.ctc_loss rejects a batch with an utterance that cannot be aligned (InvalidArgument,
 * speech_model.py:74) and the failing sess.run then touches no variable (speech_model.py:82).  Here the CTC
 * kernel reports such utterances in `status`; st_ctc_status_gate_f32 folds the status words into one device float
 * (the number of bad utterances; data-parallel training all-reduces it with the gradients), and the update
 * becomes a no-op -- params, m and v untouched, stats still written -- when *gate != 0.  gate == NULL: ungated.
 * The update is also skipped when the global norm is not finite (stats[0] then holds the NaN / Inf): a poisoned gradient never
 * reaches params, m or v. */
int st_ctc_status_gate_f32(const int32_t* status, int batch, float* gate, void* stream);
/* ... and this rank's share of the GLOBAL mean loss (speech_model.py:75 reduce_mean) in gate[1] = sum_b (loss_hi[b] + loss_lo[b]) *
 * loss_scale (summed in double; loss_lo may be NULL; loss_scale = 1 / global batch): gate[0..1] sit inside the first gradient
 * bucket, so data-parallel training gets the mean loss out of the gradient exchange itself -- no scalar all-reduce per step. */
int st_ctc_status_gate_loss_f32(const int32_t* status, int batch, const float* loss_hi, const float* loss_lo, float loss_scale,
                                float* gate, void* stream);
int st_global_norm_clip_adam_gated_f32(float* params, const float* grads, float* m, float* v, size_t n,
                                       float clip_norm, float lr_t, float beta1, float beta2, float eps,
                                       float* stats, const float* gate, void* workspace,
                                       size_t workspace_bytes, void* stream);
/* Counted form: the number of updates applied lives on the device, so that a skipped update (gate, non-finite norm) can never
 * advance the bias correction.  counts (device, 2 x uint32): counts[0] = updates applied so far, counts[1] = updates skipped
 * because the global norm was not finite.  The update uses t = counts[0] + 1, lr_t = lr * sqrt(1 - beta2^t) / (1 - beta1^t)
 * computed in double (the host formula, rounded to float once), and the moments use (float)beta1 / (float)beta2.  Afterwards
 * counts[0] += 1 if the update was applied, counts[1] += 1 if the norm was not finite; a gated update moves neither.  stats
 * (device, 3 floats, or NULL) receives {global_norm, scale, lr_t}; gate as in the gated form (NULL: ungated).  The update itself
 * is the gated form's arithmetic: given the same lr_t, the two write the same bits.  Workspace: st_global_norm_ws(n) bytes (the
 * other forms need NORM_BLOCKS floats of it only). */
int st_global_norm_clip_adam_counted_f32(float* params, const float* grads, float* m, float* v, size_t n,
                                         float clip_norm, double lr, double beta1, double beta2, float eps,
                                         float* stats, const float* gate, uint32_t* counts, void* workspace,
                                         size_t workspace_bytes, void* stream);
/* norm only (stats[0] = ||g||, stats[1] = clip/max(norm,clip)); used for reporting */
int st_global_norm_f32(const float* grads, size_t n, float clip_norm, float* stats,
                       void* workspace, size_t workspace_bytes, void* stream);

/* ---- K1-K3: calc_power_spectrogram (preprocessing.py:36-58) -----------------------------
 * audio: concatenated float samples, sample_offsets [n_utts+1].  For every utterance:
 * reflect-pad, Hann-512 STFT with hop, |.|^2, mel_basis [n_mels][n_fft/2+1], power_to_db with
 * ref = max, top_db 80, then (x-mean)/std over the whole matrix, written transposed as
 * out[frame_offsets[u] + t][n_mels] (frames = 1 + len/hop).  max_samples = longest utterance
 * (each must exceed n_fft/2 samples, numpy reflect padding); total_frames = frame_offsets[n_utts]. */
/* Planned form: the sparse mel filterbank is compiled once per (sample rate, n_mels) into a device-side plan
 * (st_melspec_plan_bytes() bytes, 16-byte aligned) and st_melspec_planned_f32 runs without touching mel_basis;
 * st_melspec_f32 is the one-call form that rebuilds the plan inside its workspace on every call. */
size_t st_melspec_plan_bytes(void);
int st_melspec_plan_f32(const float* mel_basis, int n_mels, int n_fft, void* plan, size_t plan_bytes, void* stream);
int st_melspec_planned_f32(const float* audio, const int64_t* sample_offsets, int n_utts, int64_t max_samples,
                           const void* plan, int n_mels, int n_fft, int hop, const int64_t* frame_offsets,
                           int64_t total_frames, float* out, void* workspace, size_t workspace_bytes, void* stream);
size_t st_melspec_ws(int n_utts, int64_t total_frames, int n_mels);
int st_melspec_f32(const float* audio, const int64_t* sample_offsets, int n_utts, int64_t max_samples,
                   const float* mel_basis, int n_mels, int n_fft, int hop,
                   const int64_t* frame_offsets, int64_t total_frames, float* out, void* workspace,
                   size_t workspace_bytes, void* stream);

/* ---- bf16 activations (BASELINE config 4: "bf16 activations / fp32 CTC") ------------------
 * Additional symbols, not a second code path for fp32.  Activations and activation gradients are
 * stored in HBM as bf16 (round-to-nearest-even) with the SAME padded NWC geometry as the fp32
 * tensors: every entry point takes the st_tensor3 for the geometry (its `base` is ignored) and a
 * separate pointer to the bf16 data.  Filters stay fp32 masters (packed layout above) with a
 * transposed bf16 copy [n_pad][k_pad] made by st_filters_bf16 (k_pad, n_pad from st_packed_dims;
 * the back-prop operand comes from st_filters_bwd_bf16).
 * Accumulation, bias, ReLU, the logits of the last layer, CTC, clip and Adam are fp32.
 *   forward : y = relu?(conv(x) + bias) -> y_bf16 and/or y_f32 (either may be NULL)
 *   bwd-data: dx = conv^T(dz) * [act > 0]  (stride-1 layers; act = the layer input, NULL = no mask);
 *             workspace of st_conv1d_bwd_data_bf16_ws bytes (0 for most shapes: only long reductions
 *             on few output tiles are split into fp32 partial sums)
 *   bwd-filt: dpacked [k_pad][n_pad] (rows < width*c_pitch written) and dbias [n_pad], fp32;
 *             stride 1 or 2; workspace from st_conv1d_bwd_filter_bf16_ws. */
int st_cast_bf16(const float* src, size_t n, void* dst, void* stream);
int st_filters_bf16(const float* packed, int k_pad, int n_pad, void* wt, void* stream);
/* back-prop operand [n_pad(cin)][k_pad(width*cout_pitch)] (zero-initialised by the caller) straight from
 * the packed filters: out[c][(W-1-w)*cout_pitch + o] = packed[w*cin_pitch + c][o] */
int st_filters_bwd_bf16(const float* packed, int width, int cin, int cout, int cin_pitch, int cout_pitch,
                        void* wtt, void* stream);
int st_conv1d_nwc_fwd_bf16(const st_tensor3* x, const void* x_bf16, const void* wt_bf16,
                           const float* bias, int width, int stride, int pad_left, int relu,
                           const st_tensor3* y, void* y_bf16, float* y_f32, void* stream);
/* same with a workspace (st_conv1d_fwd_bf16_ws bytes): few output rows split the reduction, as in
 * st_conv1d_nwc_fwd_ws_f32 */
size_t st_conv1d_fwd_bf16_ws(const st_tensor3* x, const st_tensor3* y, int width);
int st_conv1d_nwc_fwd_ws_bf16(const st_tensor3* x, const void* x_bf16, const void* wt_bf16,
                              const float* bias, int width, int stride, int pad_left, int relu,
                              const st_tensor3* y, void* y_bf16, float* y_f32, void* workspace,
                              size_t workspace_bytes, void* stream);
size_t st_conv1d_bwd_data_bf16_ws(const st_tensor3* dz, const st_tensor3* dx, int width);
int st_conv1d_nwc_bwd_data_bf16(const st_tensor3* dz, const void* dz_bf16, const void* wtt_bf16,
                                int width, int pad_left, const st_tensor3* act, const void* act_bf16,
                                const st_tensor3* dx, void* dx_bf16, void* workspace,
                                size_t workspace_bytes, void* stream);
size_t st_conv1d_bwd_filter_bf16_ws(const st_tensor3* x, const st_tensor3* dz, int width, int stride,
                                    int pad_left);
int st_conv1d_nwc_bwd_filter_bf16(const st_tensor3* x, const void* x_bf16, const st_tensor3* dz,
                                  const void* dz_bf16, int width, int stride, int pad_left,
                                  float* dpacked, float* dbias, void* workspace,
                                  size_t workspace_bytes, void* stream);
/* The same for STRIDE-1 layers without the reduction-major copies: both planes are staged as they lie in HBM and transposed on
 * their way from LDS into the matrix registers (ds_read_b64_tr_b16, csrc/wgrad_tr_bf16.hip).  Preconditions beyond the entry
 * point above: stride 1, x->t_pitch == dz->t_pitch (always true for a 'SAME' layer laid out as the header describes), and both
 * planes READABLE AND ZERO for st_conv1d_bwd_filter_tr_bf16_slack_rows() rows behind their last row.  _ws returns 0 for a
 * geometry the entry point does not take. */
int st_conv1d_bwd_filter_tr_bf16_slack_rows(void);
size_t st_conv1d_bwd_filter_tr_bf16_ws(const st_tensor3* x, const st_tensor3* dz, int width, int stride, int pad_left);
int st_conv1d_nwc_bwd_filter_tr_bf16(const st_tensor3* x, const void* x_bf16, const st_tensor3* dz, const void* dz_bf16,
                                     int width, int stride, int pad_left, float* dpacked, float* dbias, void* workspace,
                                     size_t workspace_bytes, void* stream);

/* ---- gradient exchange (RCCL over xGMI) ---------------------------------
 * The reference is single-replica (training.py:46); data parallelism follows from
 * speech_model.py:75-82 (mean loss over the batch, clip and Adam on the mean gradient).  One
 * communicator per process.  Rank 0 creates the id, the host moves its bytes to the other ranks,
 * every rank calls st_comm_init (collective).  st_allreduce_f32 SUMS in place, asynchronously on
 * `stream`; the bucket form groups several slices of one flat buffer into a single RCCL launch. */
int st_comm_unique_id_bytes(void);
int st_comm_unique_id(void* id_out, size_t id_bytes);
int st_comm_init(const void* id, size_t id_bytes, int rank, int world, void** comm_out);
int st_comm_destroy(void* comm);
/* ranks in the communicator as RCCL itself counts them (ncclCommCount): bench.py prints it beside torch.distributed's world size */
int st_comm_count(void* comm, int* count);
int st_allreduce_f32(void* comm, float* buf, size_t n, void* stream);
int st_allreduce_buckets_f32(void* comm, float* base, const size_t* starts, const size_t* counts, int n_buckets,
                             void* stream);

/* ---- calc_mfccs (preprocessing.py:61-84): librosa.feature.mfcc + delta + delta-delta ----------
 * Same input conventions as st_melspec_f32 (mel_basis is the n_mels = 128 filterbank librosa's
 * mfcc uses by default).  out [total_frames][3 * n_mfcc]: mfcc | delta | delta2, each block
 * z-normalised per utterance.  delta follows the librosa 0.5.x FIR implementation (see oracle). */
size_t st_mfcc_ws(int n_utts, int64_t total_frames, int n_mels, int n_mfcc);
int st_mfcc_f32(const float* audio, const int64_t* sample_offsets, int n_utts, int64_t max_samples,
                const float* mel_basis, int n_mels, int n_mfcc, int n_fft, int hop,
                const int64_t* frame_offsets, int64_t total_frames, float* out, void* workspace,
                size_t workspace_bytes, void* stream);

/* ---- kaiser_best resampling (librosa.load's implicit resample, preprocessing.py:169) ----------
 * resampy's band-limited interpolation (filter kaiser_best) + librosa's fix_length for a batch of utterances of mixed source
 * rates: `in` holds the concatenated float32 mono samples, utterance u at [in_offsets[u], in_offsets[u+1]) with source rate
 * rates[u] (int32); out utterance u at [out_offsets[u], out_offsets[u+1]) at rate sr_new.  The host plans every length
 * (audio_io.plan_resample: target = ceil(n * sr_new / sr_orig) and out_valid[u] = min(int(n * ratio), target) samples
 * interpolated, zeros after them); an utterance with rates[u] == sr_new is copied bit for bit.  win: the float64 right half
 * window (audio_io._kaiser_best_filter, win_len = 32 769 entries).  Tap selection and weights are the float64 expressions of
 * csrc/resample_map.h, shared with the host form; accumulation in float64.  All of these are device pointers.
 * st_resample_kaiser_host: the same computation on host pointers, float64 out (tests without a GPU). */
int st_resample_kaiser_f32(const float* in, const int64_t* in_offsets, int n_utts, const int32_t* rates, int sr_new,
                           const int64_t* out_offsets, const int64_t* out_valid, int64_t total_out, const double* win,
                           int64_t win_len, float* out, void* stream);
int st_resample_kaiser_host(const float* in, const int64_t* in_offsets, int n_utts, const int32_t* rates, int sr_new,
                            const int64_t* out_offsets, const int64_t* out_valid, const double* win, int64_t win_len, double* out);

/* ---- kaiser_best resampling of live streams (csrc/resample_stream.hip) ------------------------------------------------------
 * One step for all streams; the concatenated outputs of a stream's steps are st_resample_kaiser_f32's samples of the whole
 * signal, bit for bit, however the audio was cut (the arithmetic and its order are csrc/resample_map.h's, shared).  With
 * ratio = sr_new / rate and L = 32 769 / int(min(1, ratio) * 512), the most taps of a wing (64 when up-sampling, 139 for
 * 48 000 -> 22 050), output i of a stream that has received N samples is final iff int((double)i / ratio) + 1 + L <= N; once m
 * outputs are out the first sample still needed is max(int(m / ratio) - L, 0).  A finished stream emits the rest up to
 * out_valid = min(int(n_orig * ratio), target) and zeros up to target = ceil(n_orig * sr_new / rate) (audio_io.resample_lengths).
 * rate == sr_new: a copy, L = 0.  The host keeps the counters (audio_io.resample_ready / resample_need) and passes
 *   table int64 [max_streams][16], a HOST pointer (the launch is sized from it -- LDS from the ratios, grid from the counts -- and
 *   it is copied to the head of `state` in stream order; pinned memory keeps that copy asynchronous):
 *     {source rate (fixed per stream; 0: the stream sits this step out and is not touched),
 *      base0: absolute sample at position 0 of the current window, base1: of the window the step leaves,
 *      n0: samples received before the step, offset of the new samples in `samples`, their count,
 *      first output index, outputs, their offset in `out`,
 *      finished (0 / 1), n_orig, out_valid, target (read when finished),
 *      parity: which of the stream's two windows is current (the step leaves the other one current), 0, 0}
 *   state: st_resample_stream_state_bytes(max_streams, cap_samples) bytes, 8-byte aligned: the table's device copy, then two windows
 *     of cap_samples floats per stream, used in turn.  A step reads the samples [base0, n0) from the current window and the new ones
 *     from `samples`, and writes [base1, n0 + count) to the other window: no workgroup writes what another reads, nothing moves in
 *     place.  At most 2 L + 1 samples are retained, whatever the feed.  Any content before a stream's first step (n0 = base0 = 0).
 *   status int32 [max_streams]: 0, or why the row was refused -- 1 a negative or oversized field, 2 a window that would overrun
 *     cap_samples or bases out of order, 3 outputs that need samples before base0 (or a base1 the next step would miss), 4 counts
 *     that contradict the readiness rule, 5 outputs past out_capacity, 6 a tile span the LDS cannot hold.  A refused row writes no
 *     output and no state; the other rows are served.  No read leaves the windows whatever a row says; `samples` must hold
 *     [offset, offset + count) of every row.
 *   out float32 [out_capacity]: laid out as the `samples` argument of st_melspec_stream_f32, which can read it in place.
 * One launch: a workgroup per (stream, 256 outputs) stages the tile's source span (ceil(256 / ratio) + 2 L + 2 floats) in LDS, one
 * thread per output walks its wings against it; a stream whose span exceeds 64 KiB is an error and nothing is launched.
 * st_resample_stream_host: the same step on HOST pointers (state included), no GPU; it also writes the float64 sums to out64, which
 * compare with st_resample_kaiser_host. */
size_t st_resample_stream_state_bytes(int max_streams, int cap_samples);
int st_resample_stream_f32(const float* samples, const int64_t* table, int max_streams, int sr_new, const double* win, int64_t win_len,
                           void* state, size_t state_bytes, int cap_samples, float* out, int64_t out_capacity, int32_t* status,
                           void* stream);
int st_resample_stream_host(const float* samples, const int64_t* table, int max_streams, int sr_new, const double* win, int64_t win_len,
                            void* state, size_t state_bytes, int cap_samples, float* out, double* out64, int64_t out_capacity,
                            int32_t* status);

/* ---- Silence segmentation: cut recordings into utterances (csrc/segment.hip) ------------------------------------------------
 * The endpointing of the reference's `record` (record_utils.AudioRecorder: normalise the peak to 0.5, trim samples with
 * abs(x) <= threshold from both ends, add 0.1 s of zeros on each side) applied to whole recordings.  Input layout of
 * st_resample_kaiser_f32: concatenated float32 mono signals, offsets int64 [n + 1], rates int32 [n]; finite samples.
 *
 * Rules (the numpy specification, in integer and float32 arithmetic only, is tests/segment_oracle.py; the device matches it bit
 * for bit):
 *  1. peak_i = max |x| over signal i; thr_i = threshold2 * peak_i, one float32 product, with threshold2 = float32(2 * threshold)
 *     (the reference's threshold after its normalisation of the peak to 0.5).  A sample is ACTIVE iff |x| > thr_i (strict).  A
 *     signal with peak_i == 0, or without samples, has no segments.
 *  2. Chunks of c_i = max(1, rate_i / 50) samples (20 ms; integer division): chunk k covers [k c, min((k + 1) c, n_i)) and is
 *     active iff it holds an active sample.  Per chunk: its peak |x|, its first and its last active sample.
 *  3. A RUN is a maximal stretch from an active chunk to an active chunk without gap_chunks (G >= 1) or more consecutive silent
 *     chunks inside.
 *  4. A run longer than max_chunks (M >= 2) chunks is cut from the left, repeatedly while what is left is longer than M: among the
 *     chunks j of [start + M / 2, start + M) the one with the smallest peak (the smallest j among equals); the left piece is
 *     [start, j), the rest starts again at the first active chunk >= j.
 *  5. A piece becomes the samples from the first active sample of its first active chunk to one past the last active sample of
 *     its last active chunk.
 *  6. Gather: segment s becomes pads[s] zeros, x[start:end] * gain_s, pads[s] zeros, with gain_s = float32(0.5) / segpeak_s
 *     (a correctly rounded float32 division, then one float32 product per sample) and segpeak_s = max |x| over the segment.
 *
 * Tables.  Signal i owns the GROUPS [group_offsets[i], group_offsets[i + 1]) of 64 chunks, ceil(chunks_i / 64) of them (int64
 * [n + 1], planned by the host): chunk k of signal i is entry 64 * group_offsets[i] + k of chunk_peak / chunk_first / chunk_last
 * (offsets inside the chunk, -1 where it is silent) and bit k % 64 of word group_offsets[i] + k / 64 of chunk_mask.  All tables
 * hold 64 * total_groups entries (chunk_mask: total_groups words); audio and seg_ranges are 16-byte aligned.
 *  st_segment_chunks_f32: rules 1-2 (two launches); peaks [n] receives peak_i.
 *  st_segment_runs: rules 3-5, one wavefront per signal.  The segments of signal i are rows 64 * group_offsets[i] ... of
 *    seg_ranges [.][2] (start, end: samples inside the signal) and seg_peaks (segpeak: the largest chunk peak of the piece, which
 *    an active sample attains) in time order, seg_counts[i] of them -- never more than the signal has active chunks.
 *  st_segment_gather_f32: rule 6 for n_segments segments: src_start[s] = index of the segment's first sample in `audio`,
 *    seg_peaks[s], out_offsets int64 [n_segments + 1] with out_offsets[s + 1] - out_offsets[s] = 2 * pads[s] + length.
 * Every output is written with ordinary vector stores; no workspace. */
int st_segment_chunks_f32(const float* audio, const int64_t* offsets, const int32_t* rates, const int64_t* group_offsets,
                          int n_signals, int64_t total_groups, float threshold2, float* peaks, float* chunk_peak,
                          int32_t* chunk_first, int32_t* chunk_last, uint64_t* chunk_mask, void* stream);
int st_segment_runs(const int64_t* offsets, const int32_t* rates, const int64_t* group_offsets, int n_signals, int gap_chunks,
                    int max_chunks, const float* chunk_peak, const int32_t* chunk_first, const int32_t* chunk_last,
                    const uint64_t* chunk_mask, int64_t* seg_ranges, float* seg_peaks, int32_t* seg_counts, void* stream);
int st_segment_gather_f32(const float* audio, const int64_t* src_start, const float* seg_peaks, const int64_t* out_offsets,
                          const int32_t* pads, int n_segments, int64_t total_out, float* out, void* stream);

/* ---- Masked batches: zero the rows t >= valid[b] (t < frames) of every batch row b of a padded NWC tensor, over the whole
 * c_pitch, in 16-byte stores.  elem_bytes 4: the float tensor at t->base; 2: a bf16 plane of the same geometry at t->base.
 * A forward pass that does this after every layer with valid[b] = ceil(seq_len_b / strides so far) gives a batched utterance
 * the SAME padding it would see alone (engine.forward(mask_padding=True)). */
int st_mask_rows(const st_tensor3* t, const int32_t* valid, int elem_bytes, void* stream);

/* ---- Streaming recognition (csrc/conv_stream.hip, csrc/stream_map.h; no reference counterpart): one step of the forward pass
 * for many open streams, state carried between steps.  Every layer keeps per stream a linear window of recent input frames,
 * windows[max_streams][cap][cin_pitch]; position 0 of stream s holds absolute input frame info[s][0].  The per-stream counters are
 * pure functions of how many frames were fed, so the HOST keeps them (speecht_amd/streaming.py `plan`) and passes tables:
 *   info  int32 [max_streams][4]  {base: absolute frame at window position 0, n: frames received (valid frames are [0, n)),
 *                                  base after this step, unused}
 *   rows  int32 [n_rows][2]       (stream, absolute output frame), a stream's rows adjacent and in frame order
 * st_stream_conv_f32: one layer, one step, all streams.  Row (s, j) reads the frames j * stride - pad_left ... + width - 1 of stream
 *   s (pad_left = (width - stride) / 2; frames outside [0, n) and outside the window read as zero), against the engine's packed
 *   filters [k_pad][n_pad] and bias [n_pad]; bias and optional ReLU applied.  With out_info (the NEXT layer's info table) the result
 *   goes to out[s][j - out_info[s][0]][out_pitch], channels [cout, out_pitch) as zeros; with out_info NULL row r of the launch goes
 *   to out[r][out_pitch] (out_cap rows: the logits buffer).  The reduction is cut into `slices` slices of kt_per_slice 32-deep k-tiles
 *   (st_stream_conv_slices: a function of width, cin_pitch and cout only), partial tiles go to the workspace
 *   (st_stream_conv_ws bytes for n_rows rows) and a second kernel sums them in slice order: a row's result does not depend on the
 *   other rows of the launch, their number or its own position.  No float atomics.  n_rows = 0 enqueues nothing.
 * st_stream_feed_f32: row r of features [n_rows][channels] to position table[r][1] of stream table[r][0]'s first-layer window
 *   (pad channels as zeros).
 * st_stream_advance: for every layer l < n_layers and stream, moves frames [info[l][s][2], info[l][s][1]) to the front of the window;
 *   layer_table is a DEVICE table of n_layers entries {float* windows, int32 cap, int32 c_pitch}, info int32 [n_layers][max_streams][4].
 * st_ctc_greedy_stream: greedy CTC decoding carried across steps, one wavefront per stream.  table int32 [max_streams][4] =
 *   {first row, rows, decode limit or -1 while unknown, 1: reset the stream's state first}; rows with frame >= limit are not decoded.
 *   state int32 [max_streams][4] {last argmax id, frames decoded, -, -} and score double [max_streams] (sum of the chosen logits)
 *   persist between calls.  First maximum on ties, columns below num_classes only, blank = num_classes - 1, repeats merged across
 *   calls.  New ids go to ids[s][max_new], their number to new_count[s], the running negative sum to neg_sum_logits[s]. */
int st_stream_conv_slices(int width, int cin_pitch, int cout, int* kt_per_slice, int* slices);
size_t st_stream_conv_ws(int n_rows, int width, int cin_pitch, int cout);
int st_stream_conv_f32(const float* windows, int cap, int cin_pitch, const int32_t* info, const int32_t* rows, int n_rows,
                       int max_streams, const float* packed, const float* bias, int width, int stride, int cout, int relu,
                       float* out, int out_cap, int out_pitch, const int32_t* out_info, void* workspace, size_t workspace_bytes,
                       void* stream);
int st_stream_feed_f32(const float* features, int channels, const int32_t* table, int n_rows, int max_streams, float* windows,
                       int cap, int cin_pitch, void* stream);
int st_stream_advance(const void* layer_table, int n_layers, const int32_t* info, int max_streams, void* stream);
int st_ctc_greedy_stream(const float* logits, int pitch, int num_classes, const int32_t* rows, const int32_t* table, int max_streams,
                         int32_t* state, double* score, int32_t* ids, int max_new, int32_t* new_count, float* neg_sum_logits,
                         void* stream);

/* ---- Beam search carried across steps (csrc/ctc_beam.hip: ctc_beam_kernel<.., STREAM>, ctc_beam_read_kernel).  The prefix beam
 * searches of st_ctc_beam_search_decode_ex / _lm, one wavefront per stream, with everything that lives across frames kept in a
 * per-stream state record between calls, so that a stream decoded in steps IS the whole-utterance search on the concatenated rows:
 * ids, length and log_prob are bit-identical however the rows were cut.  lm NULL: the LM-free search (2..32 classes); with a model
 * (uploaded to the stream's device) the classes are a-z ' space blank (29) and one weight triple applies.  Beams 1..128.
 *   state  max_streams records of st_ctc_beam_stream_state_bytes(beam_width, lm != NULL) bytes, 8-byte aligned: a 32-byte header
 *          {magic, live entries, frames decoded, status, stable_len, -, double offset}, the live beam set (40 B per entry of 64 or,
 *          above beam 64, 128) and with a model each entry's LM state (44 B) and 28 expansion deltas (128 B).  Any content before a
 *          stream's first step, which carries reset = 1; a record never reset for this beam width and kind is left alone.
 *   pool   max_streams node pools of st_ctc_beam_stream_pool_bytes(max_frames, beam_width) bytes: (parent, label) pairs, the pair
 *          of frame t and rank r at 1 + t * beam_width + r with t the stream's ABSOLUTE frame index.  A frame at or beyond
 *          max_frames is NOT decoded: status bit 0 is set in the record instead and nothing is written outside the pool.
 *   rows, table  the tables of st_ctc_greedy_stream: rows int32 [n_rows][2] (stream, absolute frame), table int32 [max_streams][4]
 *          {first row, rows, decode limit or -1, reset}; row r of the launch is logits[r * pitch].  Rows at or past the limit are
 *          not decoded.
 * st_ctc_beam_stream_step: the log-softmax of the step's rows (the arithmetic of the whole-utterance searches, input_transform as
 *   there) into the workspace (st_ctc_beam_stream_ws(n_rows) bytes), then the frames of every stream; no tail, no output.
 * st_ctc_beam_stream_read: for every stream with rows in the step, a reset or a limit >= 0 (the others' outputs stay untouched):
 *   stable_len, the length of the longest common prefix -- compared by labels -- of all live entries: every later entry extends a
 *   live one, so these labels are final.  The kernel walks the chains down to the stored stable_len only and stores the new one.
 *   The reported hypothesis is entry 0 of the set (running total, no end-of-utterance terms) while the stream is open and, once
 *   limit >= 0, exactly the whole-utterance result: with a model every entry gains lm_weight * (incomplete word, then </s>) and the
 *   best total wins, ties to the lower rank.  result int32 [max_streams][4] = {length of the hypothesis, new stable_len, log_prob
 *   (float bits), status: bit 0 pool full, bit 1 no state}; tail[s][i] = label (old stable_len + i) of the hypothesis, i < max_tail.
 *   The caller keeps the labels below stable_len from earlier reads. */
size_t st_ctc_beam_stream_state_bytes(int beam_width, int lm);
size_t st_ctc_beam_stream_pool_bytes(int max_frames, int beam_width);
size_t st_ctc_beam_stream_ws(int max_rows);
int st_ctc_beam_stream_step(const float* logits, int pitch, int num_classes, const int32_t* rows, const int32_t* table, int n_rows,
                            int max_streams, int beam_width, int input_transform, void* lm, float lm_weight, float word_count_weight,
                            float valid_word_count_weight, float oov_score, void* state, void* pool, int max_frames, void* workspace,
                            size_t workspace_bytes, void* stream);
int st_ctc_beam_stream_read(const int32_t* table, int max_streams, int beam_width, void* lm, float lm_weight, float word_count_weight,
                            float valid_word_count_weight, float oov_score, void* state, const void* pool, int max_frames,
                            int32_t* tail, int max_tail, int32_t* result, void* stream);

/* ---- Endpointing of live streams (csrc/stream_endpoint.hip, csrc/stream_endpoint_core.h; specification: tests/endpoint_oracle.py; no
 * reference counterpart).  The device notices that a speaker has stopped, closes the utterance and steers the decoders above, so that
 * a stream of any length is a sequence of utterances decoded like files.  The rule is a pure function of a stream's logits rows:
 * row t is SILENT when its argmax -- computed as st_ctc_greedy_stream computes it -- is the blank (num_classes - 1) or space_id (-1: no
 * such class), SPEECH otherwise.  With R = silence_frames >= 1, L = lead_frames >= 1, M = max_frames >= L: row t always joins the open
 * utterance [u0, ...); a speech row sets started and run = 0, a silent row increments run; then, with len = t + 1 - u0, the first of
 *   1 silence: started && run >= R;   2 length: started && len >= M;   3 discard: !started && len >= L
 * that applies fires; 1 and 2 make the utterance [u0, t + 1) final, 3 drops the rows (no utterance), and after any of them u0 = t + 1,
 * started = false, run = 0.  When the stream finishes (limit >= 0; rows at or past the limit are not consumed) a non-empty open stretch
 * ends with event 4 (end of stream) if it has started and with event 3 otherwise.  No stretch is longer than M rows.
 * st_stream_endpoint_pieces: P = 2 + (max_rows - 1) / min(L, R + 1, M), the event and piece slots per stream for steps of at most
 *   max_rows rows per stream (0: bad arguments); st_stream_endpoint_state_bytes / _score_bytes: bytes of one stream's record / score.
 * st_ctc_greedy_endpoint_stream: one wavefront per stream, in the place of st_ctc_greedy_stream (same logits, rows and table).  Greedy
 *   decoding restarts at every event, so an utterance's ids and sum are those of its rows alone.
 *   state   int32 [max_streams][8] {u0, started, run, first_speech, last_speech, finals so far, last argmax id, rows consumed} and
 *           score float [max_streams][256] (the open utterance's chosen logits: row i of the utterance is added to slot i % 256, and a
 *           sum is the binary tree of neighbours over the slots -- the order of st_ctc_greedy_decode, whose neg_sum_logits on an
 *           utterance's rows a final's therefore equals bit for bit) persist between calls; any content before a stream's first step,
 *           which carries reset = 1 (frames count from 0 then).
 *   ids     [max_streams][max_new]: all new ids of the step, the utterances' concatenated; new_count[s] their number;
 *           neg_sum_logits[s] the negative sum of the utterance still open.
 *   events  int32 [max_streams][n_pieces][8] = {kind (0 ends the list; all n_pieces slots may be in use), u0, end, first_speech or -1,
 *           last_speech or -1, ids_end: this step's ids up to the end of this stretch, negative sum of its chosen logits (float bits),
 *           utterance index (of a discard: the index the next final will get)}
 *   pieces  int32 [n_pieces][max_streams][4], each pieces[p] a table {first row, rows, limit, reset} of the streaming decoders: the
 *           step's rows of one stretch.  The piece that ends a final utterance carries limit = its end frame (absolute, as the rows
 *           table counts), every other one -1; the piece after an event -- and the first one of a step the host marked reset --
 *           carries reset = 1, also when it has no rows yet (an event on a step's last row: {0, 0, -1, 1}); a final at the end of the
 *           stream whose rows all came earlier is {0, 0, end, 0}; a stream without rows and unused slots are {0, 0, -1, 0}.  Pieces
 *           lie inside the host's [first, first + rows).  Slots from n_pieces on are never written; n_pieces below
 *           st_stream_endpoint_pieces(max_rows, ...) is refused, and a table row with more than max_rows rows loses its later events.
 * st_stream_endpoint_host: the same on HOST pointers, bit-identical to the kernel (one walk, csrc/stream_endpoint_core.h).  No GPU.
 * st_ctc_beam_stream_step_pieces (csrc/ctc_beam.hip): st_ctc_beam_stream_step's log-softmax of the step's rows once, then for p = 0 ..
 *   n_pieces - 1 the search of st_ctc_beam_stream_step with table = pieces[p] followed by the read-out of st_ctc_beam_stream_read into
 *   result[p] ([n_pieces][max_streams][4]) and tail[p] ([n_pieces][max_streams][max_tail]; relative to the stable length the read
 *   before it stored, 0 after a reset).  The tables are read on the device: no host wait.  A final piece's read-out is the
 *   whole-utterance search on the utterance's rows, bit for bit; with max_frames = M the pool-full status bit never sets. */
size_t st_stream_endpoint_state_bytes(void);
size_t st_stream_endpoint_score_bytes(void);
int st_stream_endpoint_pieces(int max_rows, int silence_frames, int lead_frames, int max_frames);
int st_ctc_greedy_endpoint_stream(const float* logits, int pitch, int num_classes, const int32_t* rows, const int32_t* table,
                                  int max_streams, int space_id, int silence_frames, int lead_frames, int max_frames, int max_rows,
                                  int32_t* state, float* score, int32_t* ids, int max_new, int32_t* new_count, float* neg_sum_logits,
                                  int32_t* events, int32_t* pieces, int n_pieces, void* stream);
int st_stream_endpoint_host(const float* logits, int pitch, int num_classes, const int32_t* rows, const int32_t* table, int max_streams,
                            int space_id, int silence_frames, int lead_frames, int max_frames, int max_rows, int32_t* state,
                            float* score, int32_t* ids, int max_new, int32_t* new_count, float* neg_sum_logits, int32_t* events,
                            int32_t* pieces, int n_pieces);
int st_ctc_beam_stream_step_pieces(const float* logits, int pitch, int num_classes, const int32_t* rows, const int32_t* pieces,
                                   int n_pieces, int n_rows, int max_streams, int beam_width, int input_transform, void* lm,
                                   float lm_weight, float word_count_weight, float valid_word_count_weight, float oov_score, void* state,
                                   void* pool, int max_frames, void* workspace, size_t workspace_bytes, int32_t* tail, int max_tail,
                                   int32_t* result, void* stream);

/* ---- Word times and confidences for the finals of live streams (csrc/stream_words.hip, csrc/stream_ring.h, and the ring entry
 * points in csrc/ctc_align.hip / csrc/ctc_conf.hip; no reference counterpart).  A stream's logits buffer holds one step's rows, so the
 * rows of an utterance the endpointer closes are gone by then.  The recogniser keeps them in a ring per stream,
 *   ring   float [max_streams][cap][32]: frame f of stream s at ring[s][f % cap]; columns at and past num_classes are never read,
 * and the alignment and confidence lattices read a final's rows back from there: what they return is what st_ctc_align_f32 /
 * st_ctc_word_conf_f32 return on the utterance's rows alone, bit for bit.
 * st_stream_keep_rows: cap = max_frames + max_rows, the rows per stream the ring must hold for utterances of at most max_frames rows
 *   (the endpointer's M) and passes of at most max_rows rows per stream; 0 on bad arguments (either below 1).  Why that is enough: no
 *   stretch is longer than M rows (the endpoint rule), so a final is [u0, end) with end - u0 <= M; finals are aligned in the pass that
 *   closes them, before the next pass keeps anything; and that pass holds at least the row end - 1, so it has kept fewer than max_rows
 *   rows behind end.  The newest frame kept is therefore below u0 + M + max_rows - 1 = u0 + cap - 1: no slot of [u0, end) has been
 *   written twice.
 * st_stream_keep_f32: one launch; for every entry (stream, frame) of the step's last-layer `rows` table (int32 [n_rows][2], the table
 *   of st_ctc_greedy_stream) row i of logits -- logits[i * pitch + 0 .. num_classes) -- goes to ring[stream][frame % cap].  Frame
 *   numbers are the table's own, the ones the endpoint events report; they start at 0 after a reset, so a reused slot needs no
 *   clearing.  1 <= num_classes <= 32, pitch >= num_classes.  An entry with a stream outside 0 .. max_streams - 1 or a negative
 *   frame is skipped.  n_rows = 0 is valid and launches nothing.  Enqueues only, never allocates; ordinary vector loads and stores,
 *   one lane per float.
 * st_ctc_align_ring_f32: the semantics of st_ctc_align_f32 for a batch of n_jobs utterances whose rows live in the ring.
 *   jobs   DEVICE int32 [n_jobs][3] = {stream, u0, n_rows}: row t of job j is ring[stream_j][(u0_j + t) % cap], seq_lens[j] = n_rows_j,
 *          frames = max_rows (given by the caller: the pitch of `states` and of the workspace).
 *   Labels CSR over the jobs, 2 <= num_classes <= 32; spans, states (may be null), score, status and the workspace,
 *   st_ctc_align_ws(n_jobs, max_rows, max_label_len) bytes, exactly as there.  A job with stream outside 0 .. max_streams - 1,
 *   n_rows outside 0 .. max_rows or u0 < 0 gets status != 0 (score -inf, spans {-1, -1}, states -2) and reads nothing outside the
 *   ring.  Rows t >= n_rows_j are read from the ring -- defined memory -- and ignored by the lattice, as padding rows are there.
 *   Three launches: the ring-mapped ln-softmax stage (the row offset comes from the job table and a wrap; same arithmetic, same
 *   butterfly order, so the double rows have the same bits -- this stage IS the gather, there is no copy pass), then the lattice and
 *   the back-trace kernels of st_ctc_align_f32, which read the workspace only.
 * st_ctc_word_conf_ring_f32: the same for st_ctc_word_conf_f32: jobs, space_id and word_spans (whose first column is now the job),
 *   2 <= num_classes <= 30; log_prob [n_jobs], log_conf [n_words], status [n_jobs] as there (a job the ring cannot serve: status != 0,
 *   log_prob -inf, its words NaN); workspace st_ctc_word_conf_ws(n_jobs, max_rows, max_label_len, n_jobs + n_words) bytes.
 * st_ctc_align_ring_host / st_ctc_word_conf_ring_host: the same on a HOST ring and a HOST job table: each gathers the jobs' rows
 *   through the index function the kernels use (csrc/stream_ring.h) and runs st_ctc_align_host / st_ctc_word_conf_host on them:
 *   bit-identical to the device entry points and to the dense host forms on the utterance's rows.  They need no device (and, unlike
 *   the device entry points, allocate the gathered rows). */
int st_stream_keep_rows(int max_frames, int max_rows);
int st_stream_keep_f32(const float* logits, int pitch, int num_classes, const int32_t* rows, int n_rows, int max_streams, float* ring,
                       int cap, void* stream);
int st_ctc_align_ring_f32(const float* ring, int max_streams, int cap, int num_classes, const int32_t* jobs, int n_jobs, int max_rows,
                          const int32_t* label_ids, const int32_t* label_offsets, int max_label_len, int32_t* spans, int32_t* states,
                          float* score, int32_t* status, void* workspace, size_t workspace_bytes, void* stream);
int st_ctc_align_ring_host(const float* ring, int max_streams, int cap, int num_classes, const int32_t* jobs, int n_jobs, int max_rows,
                           const int32_t* label_ids, const int32_t* label_offsets, int max_label_len, int32_t* spans, int32_t* states,
                           float* score, int32_t* status, void* workspace, size_t workspace_bytes);
int st_ctc_word_conf_ring_f32(const float* ring, int max_streams, int cap, int num_classes, const int32_t* jobs, int n_jobs,
                              int max_rows, const int32_t* label_ids, const int32_t* label_offsets, int max_label_len, int space_id,
                              const int32_t* word_spans, int n_words, double* log_prob, double* log_conf, int32_t* status,
                              void* workspace, size_t workspace_bytes, void* stream);
int st_ctc_word_conf_ring_host(const float* ring, int max_streams, int cap, int num_classes, const int32_t* jobs, int n_jobs,
                               int max_rows, const int32_t* label_ids, const int32_t* label_offsets, int max_label_len, int space_id,
                               const int32_t* word_spans, int n_words, double* log_prob, double* log_conf, int32_t* status,
                               void* workspace, size_t workspace_bytes);

/* ---- Hotword biasing of the streaming beam searches, with a phrase set per stream (csrc/ctc_beam.hip: ctc_beam_kernel<.., STREAM,
 * BIAS>, ctc_beam_read_kernel<.., BIAS>).  The three entry points above with the second scorer of st_ctc_beam_search_decode_bias_nbest
 * / _lm_bias_nbest: each takes the arguments of its unbiased form, then `bias` (the tables as there: device pointers, 1 <= n_states <=
 * 2^20; a null struct or table and n_states < 1 are refused without a launch) and `roots`, a DEVICE array int32 [max_streams].  A
 * stream decoded in steps is the biased whole-utterance search on the concatenated rows: ids, length and log_prob are those of the
 * n_best = 1 list, bit for bit, however the rows were cut.  With a model the classes are the 28 labels and the blank, as above.
 *   roots  A search that starts afresh -- table reset = 1: a stream's first step, or the piece after an endpoint event -- starts in
 *          hotword state roots[s] (clamped to [0, n_states)) with no credit lent; roots[s] is read then and only then.  This is how
 *          streams of one launch have phrase sets of their own: the caller concatenates the sets' tables, shifts set k's `next`
 *          values by the row its states begin at, so that a match of set k that returns "to the root" returns to k's first row, and
 *          names that row in roots[s] (speecht_amd/hotwords.py: HotwordSets; its set 0 is one state without gain, whose streams get
 *          the unbiased search's bits).  One table of one set: roots all 0.
 *   state  records of st_ctc_beam_stream_bias_state_bytes(beam_width, lm != NULL) bytes: the record of the unbiased search -- the same
 *          layout at the same offsets -- followed by every entry's hotword state (int32 [64 or 128]) and bself, the gain it was
 *          entered with (float [64 or 128]): 8 B per entry more.  The magic carries a bias bit (0x1000): a record last reset by an
 *          unbiased step is left alone by a biased one and the reverse, and the read-out of the other kind reports status bit 1.
 *   read   While a stream is open the reported hypothesis is entry 0 with its running total, which includes the credit lent to the
 *          open match.  Once limit >= 0 every live entry adds fin[state] -- after the LM's end-of-utterance terms if there is a
 *          model, and also without one -- and the best total wins, ties to the lower rank: the tail of the biased whole-utterance
 *          searches.  A final of an endpointed piece therefore forfeits the credit of a phrase the cut leaves unfinished, and the
 *          next utterance starts at roots[s] again.  stable_len is computed as above.
 * st_ctc_beam_stream_state_bytes, the unbiased entry points, their launches and their records are unchanged. */
size_t st_ctc_beam_stream_bias_state_bytes(int beam_width, int lm);
int st_ctc_beam_stream_step_bias(const float* logits, int pitch, int num_classes, const int32_t* rows, const int32_t* table, int n_rows,
                                 int max_streams, int beam_width, int input_transform, void* lm, float lm_weight, float word_count_weight,
                                 float valid_word_count_weight, float oov_score, void* state, void* pool, int max_frames, void* workspace,
                                 size_t workspace_bytes, void* stream, const st_bias_tables* bias, const int32_t* roots);
int st_ctc_beam_stream_read_bias(const int32_t* table, int max_streams, int beam_width, void* lm, float lm_weight, float word_count_weight,
                                 float valid_word_count_weight, float oov_score, void* state, const void* pool, int max_frames,
                                 int32_t* tail, int max_tail, int32_t* result, void* stream, const st_bias_tables* bias,
                                 const int32_t* roots);
int st_ctc_beam_stream_step_pieces_bias(const float* logits, int pitch, int num_classes, const int32_t* rows, const int32_t* pieces,
                                        int n_pieces, int n_rows, int max_streams, int beam_width, int input_transform, void* lm,
                                        float lm_weight, float word_count_weight, float valid_word_count_weight, float oov_score,
                                        void* state, void* pool, int max_frames, void* workspace, size_t workspace_bytes, int32_t* tail,
                                        int max_tail, int32_t* result, void* stream, const st_bias_tables* bias, const int32_t* roots);

/* ---- N-best lists for the finals of live streams (csrc/ctc_beam.hip: ctc_beam_read_nbest_kernel).  The read-out of
 * st_ctc_beam_stream_read_bias and the endpointed step of st_ctc_beam_stream_step_pieces_bias, each also writing, for every FINISHING
 * read-out (limit >= 0: `finish`, or a final of an endpointed piece), the list "N-best lists from both beam searches" above defines:
 * the list of st_ctc_beam_search_decode_nbest / _lm_nbest / _bias_nbest / _lm_bias_nbest on the utterance's rows alone -- the same
 * ranking rules, n = min(n_best, entries alive), log_prob = (float)((double)final total + offset) -- bit for bit, however the rows were
 * cut into steps.  An open stream's read-out writes no list.  Each takes the arguments of its `_bias` form, then the four below;
 * `bias` and `roots` may both be NULL: the unbiased search with the records of st_ctc_beam_stream_state_bytes (one of them NULL is
 * refused).  `result` and `tail` are written exactly as by the other forms; hypothesis 0 of a list is that top path.
 *   n_best       1 <= n_best <= beam_width.
 *   arena        DEVICE int32 [arena_words], arena_words >= 0: the records of one call, compact.  All live entries share the labels
 *                below the stable_len the record stored BEFORE this read-out (the caller holds them: it has read every earlier
 *                `tail`), so a hypothesis is stored as its labels from there on, as `tail` is, without a max_tail limit.  A record:
 *                  {stream, piece, n, old stable_len, words of this record, 0}
 *                  n pairs {length (the whole length in ids), log_prob (float bits)}, best first
 *                  the n tails back to back, length_h - old stable_len labels each
 *                piece: the index p of the piece (0 from st_ctc_beam_stream_read_nbest).  The records' order depends on arrival,
 *                their content does not: sort by (piece, stream).
 *   arena_used   DEVICE int32 [1]: zeroed by the entry point on `stream` ahead of the first launch (one more enqueue); every
 *                finishing wave adds its record's words with one atomic and writes the record only if it lies inside
 *                [0, arena_words) as a whole -- otherwise nothing of it -- so afterwards arena_used is the true demand and nothing
 *                outside the arena is ever touched.  arena_used <= arena_words: the records lie back to back in [0, arena_used).
 *                Otherwise the records that fit lie back to back from word 0 (once one reservation has passed the end, every later
 *                one has too) and the words behind them are as the caller left them -- a caller that wants to tell where they end
 *                fills the arena with a value no header has (word 5 of a header is 0) -- and the other lists are lost.  Worst case
 *                per finishing read-out: 6 + n_best * (2 + longest tail).
 * A bad argument returns the error without a launch.  The six entry points above keep their signatures, launches and records. */
int st_ctc_beam_stream_read_nbest(const int32_t* table, int max_streams, int beam_width, void* lm, float lm_weight, float word_count_weight,
                                  float valid_word_count_weight, float oov_score, void* state, const void* pool, int max_frames,
                                  int32_t* tail, int max_tail, int32_t* result, void* stream, const st_bias_tables* bias,
                                  const int32_t* roots, int n_best, int32_t* arena, int arena_words, int32_t* arena_used);
int st_ctc_beam_stream_step_pieces_nbest(const float* logits, int pitch, int num_classes, const int32_t* rows, const int32_t* pieces,
                                         int n_pieces, int n_rows, int max_streams, int beam_width, int input_transform, void* lm,
                                         float lm_weight, float word_count_weight, float valid_word_count_weight, float oov_score,
                                         void* state, void* pool, int max_frames, void* workspace, size_t workspace_bytes, int32_t* tail,
                                         int max_tail, int32_t* result, void* stream, const st_bias_tables* bias, const int32_t* roots,
                                         int n_best, int32_t* arena, int arena_words, int32_t* arena_used);

/* ---- Keyword spotting in live streams: lattices carried across steps, packed into waves (csrc/ctc_spot_stream.hip,
 * csrc/ctc_spot_stream_core.h; specification: tests/spot_stream_oracle.py; no reference counterpart).  Every step tells which of the
 * given keywords have just been said in each stream.  The rule is a pure function of a stream's logits rows, however they are cut
 * into steps and whatever the other streams do.
 *
 * The lattice, d_t(c), the cell, the tie order and end_t / s_t(2L-1) are those of st_ctc_spot_f32 above, unchanged (the arithmetic
 * is csrc/ctc_spot_core.h's: sp_ratio, sp_column, sp_cell), with t the stream's ABSOLUTE output-frame index (int32, the frame the
 * rows table names for the stream's first row of a step; the following rows of the step are the following frames).  t + 1 must
 * stay an int32: a stream may run for 2^31 - 2 frames (about 497 days at 20 ms per frame) before it has to be reset.
 * Each (stream, keyword) pair keeps across steps its 2L+1 values and starts, a pending hit {score, start, end} or none, and
 * last_end, initially 0.  With threshold a double <= 0 or -inf (NaN is refused) and hold an int32 >= 1, after the lattice update
 * of frame t, with e = end_t and a = s_t(2L-1):
 *   1. cand = e > -inf && a >= last_end && e >= threshold * (double)(t + 1 - a)     (one IEEE multiply, contraction off);
 *   2. a pending hit, cand and a >= pending.end: the pending hit is EMITTED, last_end = pending.end, nothing is pending;
 *   3. cand and (nothing pending or e >= pending.score): pending = {e, a, t + 1} -- the later frame wins among equals;
 *   4. a pending hit and t + 1 - pending.end >= hold: it is emitted, last_end = pending.end, nothing is pending.
 * When the stream finishes (the table's limit >= 0; rows at or past the limit are not consumed) a pending hit is emitted with kind 1
 * (flushed).  hold exists because the end state can stay on the last character indefinitely with the old start: "no live path
 * overlaps any more" would never fire.  Hits of one keyword never overlap; of overlapping candidates the better one stays (the
 * causal counterpart of spotting.pick_hits); every emitted (start, end, score) is a point of the offline trace: score ==
 * trace_score[end - 1], start == trace_start[end - 1].  Endpointing does NOT reset spotting: it runs on the stream's rows as they
 * are, and its frames are the stream's, not an utterance's.
 *
 * st_ctc_spot_stream_plan_bytes / st_ctc_spot_stream_plan (HOST): pack the keywords (CSR as above: ids 0 .. num_classes - 2, 1 <= L
 *   <= 511, 2 <= num_classes <= 32, n_keywords >= 1; anything else is an error / 0 bytes) into waves of 64 * KPL states, KPL =
 *   the states-per-lane dispatch of the longest keyword.  Each keyword begins on a lane boundary and never straddles waves; its two
 *   dead outer states separate it from its neighbours.  pack = 1: keywords fill a wave in order while they fit; pack = 0: one
 *   keyword per wave.  The plan is a block of int32 words (header, per wave a table of state descriptors, per keyword its place) the
 *   caller uploads, 4-byte aligned, and then names to the host copy: st_ctc_spot_stream_plan_bind(plan, device_copy).  The step
 *   functions take the HOST copy (its header gives them the dispatch and the device address without a wait); the kernel believes only
 *   a device copy whose header carries the magic value and the classes, KPL and waves it was launched for, and does nothing otherwise.
 * st_ctc_spot_stream_state_bytes(plan): bytes of one stream's state (per wave 64 * (12 KPL + 20)), 0 for no plan.  state holds
 *   max_streams of them, 8-byte aligned; any content before a stream's first step, which carries reset = 1.
 * st_ctc_spot_stream_step: logits, pitch, rows and table as st_ctc_greedy_stream takes them ({first row, rows, limit or -1, reset};
 *   only columns < num_classes are read).  A memset of counts and ONE launch, one wave per (stream, wave of the plan); enqueues only,
 *   never allocates.  A stream without rows, reset and limit is not touched: n_rows = 0 with no finishing stream changes no state.
 *   events  int32 [max_streams][max_events][8] = {keyword, start, end, kind (0, or 1: flushed), score bits lo, hi, 0, 0}, in no
 *           particular order within a stream (sort by (end, keyword)).
 *   counts  int32 [max_streams]: the TRUE number of the stream's events of this step, whatever was there before, 0 for a stream
 *           that sat out.  Beyond max_events the surplus is not written; nothing is written outside the buffers.
 * st_ctc_spot_stream_host: the same on HOST pointers (the plan needs no device copy), bit-identical events and state; it walks the
 *   keywords one by one on their own states, which cross-checks the packing.  No GPU. */
size_t st_ctc_spot_stream_plan_bytes(const int32_t* kw_ids, const int32_t* kw_offsets, int n_keywords, int num_classes, int pack);
int st_ctc_spot_stream_plan(const int32_t* kw_ids, const int32_t* kw_offsets, int n_keywords, int num_classes, int pack, void* plan,
                            int* n_waves);
int st_ctc_spot_stream_plan_bind(void* plan, const void* device_copy);
size_t st_ctc_spot_stream_state_bytes(const void* plan);
int st_ctc_spot_stream_step(const float* logits, int pitch, int num_classes, const int32_t* rows, const int32_t* table, int n_rows,
                            int max_streams, const void* plan, double threshold, int hold, void* state, int32_t* events,
                            int max_events, int32_t* counts, void* stream);
int st_ctc_spot_stream_host(const float* logits, int pitch, int num_classes, const int32_t* rows, const int32_t* table, int n_rows,
                            int max_streams, const void* plan, double threshold, int hold, void* state, int32_t* events,
                            int max_events, int32_t* counts);

/* ---- Following a known script in live streams: one long alignment lattice per stream, carried across steps in tiles
 * (csrc/ctc_follow_stream.hip, csrc/ctc_follow_core.h; specification: tests/follow_oracle.py; no reference counterpart).  Every step
 * tells where in its script each stream's speaker is now and which words have just been reached.  The rule is a pure function of a
 * stream's logits rows, however they are cut into steps and whatever the other streams do.
 *
 * A following stream has a script l of L ids, 1 <= L <= max_labels, ids 0 .. num_classes - 2, blank = num_classes - 1.  Its lattice
 * is st_ctc_align_f32's: U = 2L+1 states, v_0(u) = ly_0(class(u)) for u < 2 and -inf otherwise, v_t(u) = al_cell(v_{t-1}(u),
 * v_{t-1}(u-1), v_{t-1}(u-2), skip only between different labels, ly_t(class(u))) (csrc/ctc_align_core.h), ly_t the double ln-softmax
 * row csrc/ctc_align_softmax.h forms (same arithmetic, same butterfly order), t the stream's ABSOLUTE output frame since its last
 * reset (int32).  No back-pointers are kept.  After frame t:
 *   1. b_t = max_u v_t(u), c_t the LOWEST state attaining it, c_t = -1 if b_t = -inf;
 *   2. pos_t = (c_t + 1) >> 1, the labels the best state has entered (0 for c_t <= 0);
 *   3. g_t = g_{t-1} + max_c ly_t(c), g_{-1} = 0, double adds in frame order; fit_t = b_t - g_t <= 0: how far the script's best
 *      reading lies below the greedy reading of the same frames, and so whether the speaker is on script at all;
 *   4. m_t = min(pos_{t-K+1} .. pos_t), frames before 0 counting as 0, K = confirm frames, 1 <= K <= 16: the cursor of a Viterbi filter
 *      jumps back and forth on noise; the sliding minimum asks for K frames of agreement without depending on step boundaries;
 *   5. the words are the maximal runs of ids other than the space, word j beginning at label a_j (word_starts, increasing): word j is
 *      REACHED at the first frame t with m_t >= a_j + 1, its event {j, t}.  Several words may be reached at one frame; they are emitted
 *      in word order, each once;
 *   6. end_score_t = v_t(al_end_state(U, v_t(U-1), v_t(U-2))): what st_ctc_align_long_f32 returns as the score of rows 0 .. t, -inf
 *      while the script does not fit.
 * Rows at or past the table's limit are not consumed; nothing is flushed when a stream finishes.  Endpointing neither sees nor
 * resets the follower.
 *
 * st_ctc_follow_stream_state_bytes(max_labels): bytes of one stream's state, a multiple of 16 (a header of 128 bytes, then two
 *   columns of 896 NB + 128 doubles, NB = ceil((2 max_labels + 1) / 896)); 0 unless 1 <= max_labels <= 28671.  state holds max_streams
 *   of them, 16-byte aligned; any content before a stream's first step, which carries reset = 1 and makes the 128 column elements
 *   below state 0 -inf.  A run leaves its new column in the second buffer and its last launch copies it over the first: between
 *   steps both hold the same, and a state's bytes depend on the stream's rows alone.
 * st_ctc_follow_stream_ws(max_rows, max_labels, max_streams): bytes of the workspace (16-byte aligned) for steps of at most max_rows
 *   rows in all: max_rows * 32 * 8 + max_streams * 64 * NB * 16 + max_streams * 32 + 256.
 * st_ctc_follow_stream_step: logits, pitch, rows and table as st_ctc_greedy_stream takes them ({first row, rows, limit or -1, reset}).
 *   script_ids / script_offsets [max_streams + 1] and word_starts / word_offsets [max_streams + 1]: DEVICE CSR arrays over the slots,
 *   owned by the caller; a slot with an empty script sits out (status 2), one whose script is longer than max_labels is not followed
 *   (status 1) -- neither reads or writes its state.  max_stream_rows: the most rows any one stream has in this step (the host knows
 *   it; the tables live on the device): the step is cut into ceil(max_stream_rows / 64) runs, at least one; a stream with more rows
 *   loses them (status 4).  One softmax launch, then per run the tile kernel (one wave per (state block, stream)) and the read-out;
 *   enqueues only, never allocates.  Bad arguments return ST_EINVAL and enqueue nothing.
 *   events  int32 [max_streams][max_events][2] = {word, frame}, in order, 8-byte aligned.  Beyond max_events the surplus is not
 *           written; nothing is written outside the buffers.
 *   result  int32 [max_streams][16] = {frames consumed, c of the last frame (-1 before the first), status, the TRUE number of this
 *           step's events, fit (double bits lo, hi; -inf before the first frame), end_score (lo, hi), words reached so far, 0 ...},
 *           written for every slot.
 *   trace   NULL, or int32 [n_rows]: c_t of every consumed row, at the row's index in the launch.
 * st_ctc_follow_stream_host: the same on HOST pointers with plain loops over the whole lattice, without tiles: results and state
 *   bit-identical, which cross-checks the halo.  No GPU. */
size_t st_ctc_follow_stream_state_bytes(int max_labels);
size_t st_ctc_follow_stream_ws(int max_rows, int max_labels, int max_streams);
int st_ctc_follow_stream_step(const float* logits, int pitch, int num_classes, const int32_t* rows, const int32_t* table, int n_rows,
                              int max_rows, int max_stream_rows, int max_streams, const int32_t* script_ids,
                              const int32_t* script_offsets, const int32_t* word_starts, const int32_t* word_offsets, int max_labels,
                              int confirm, void* state, int32_t* events, int max_events, int32_t* result, int32_t* trace,
                              void* workspace, size_t workspace_bytes, void* stream);
int st_ctc_follow_stream_host(const float* logits, int pitch, int num_classes, const int32_t* rows, const int32_t* table, int n_rows,
                              int max_rows, int max_stream_rows, int max_streams, const int32_t* script_ids,
                              const int32_t* script_offsets, const int32_t* word_starts, const int32_t* word_offsets, int max_labels,
                              int confirm, void* state, int32_t* events, int max_events, int32_t* result, int32_t* trace,
                              void* workspace, size_t workspace_bytes);

/* st_melspec_stream_f32: the mel front end, one step for all streams (csrc/melspec.hip).  Frame t needs samples t * hop - 256 ...
 * t * hop + 255, reflected at the start of the stream and, at the end, once the stream is finished; every stream's sample tail stays
 * in `state` (st_melspec_stream_state_bytes; any content before a stream's first step, which carries reset = 1).  Frames are
 * transformed in the pairs (2p, 2p + 1) of the whole-utterance kernel, so a frame's log-mel power equals st_melspec_f32's bit for
 * bit and does not depend on the chunking; an open stream emits whole pairs only.  The host keeps the counters and passes
 *   table int32: [max_streams][8] {base: absolute sample at window position 0, n: samples received, base after the step, finished,
 *                                  first row of the stream among this step's frames, new frames, index of the first new frame, reset}
 *                [max_streams][4] {offset in `samples`, count, window position, -}       (the new samples of each stream)
 *                [n_pairs][2]     (stream, even frame index)
 * Causal normalisation (fixed = 0): with h(t) = max(t, warm - 1), or the last frame when the stream ends sooner, ref_t is the largest
 * mel power over frames 0 ... h(t), x_t = max(dB(S_t) - dB(ref_t), -80), mean_t and std_t the mean and population deviation of all
 * x_t', t' <= h(t), each as it was computed, and the output (x_t - mean_t) / std_t; sums in double, a frame's values in a fixed
 * tree, frames one by one.  The first `warm` frames therefore appear together, and an utterance of at most `warm` frames gets the
 * whole-utterance features.  fixed = 1: x = max(dB(S) - dB(2^ref_log2), -80), output (x - mean) / std, no running update.
 * A zero deviation is not special-cased (as in st_melspec_f32).  Stream s's frames of this step go to out[s][i][n_mels], i counting
 * from 0 (out_cap frames per stream; how many is known to the host).  Workspace: st_melspec_stream_ws for max_rows frames per step. */
size_t st_melspec_stream_state_bytes(int max_streams, int cap_samples, int n_mels, int warm);
size_t st_melspec_stream_ws(int max_rows, int n_mels);
int st_melspec_stream_f32(const float* samples, const int32_t* table, int n_pairs, int max_streams, const void* plan, int n_mels,
                          int hop, int warm, int cap_samples, int fixed, float ref_log2, float mean, float std, void* state,
                          size_t state_bytes, float* out, int out_cap, int max_rows, void* workspace, size_t workspace_bytes,
                          void* stream);

/* ---- SpecAugment while the batch is loaded (csrc/spec_augment.hip, csrc/spec_augment_core.h; no reference counterpart: the
 * reference trains without augmentation).  The copy of a staged feature batch src [batch][frames][channels] (fp32, contiguous) into
 * the padded input tensor `dst`, with every utterance's time warp, frequency masks and time masks (Park et al. 2019) applied on the
 * way: one launch, the bytes of the plain copy.  Only interior rows and the valid channels of dst are written; rows at or past an
 * utterance's seq_len get the source's rows unchanged.  Masked elements become 0 (the features are zero-mean per utterance).
 *   policy    time_warp W (largest displacement, frames; the warp applies to utterances of at least 2W + 2 frames), freq_masks
 *             masks of width 0 .. min(freq_width, channels), time_masks masks of width 0 .. min(time_width, floor(p seq_len)) with
 *             p = time_ratio_q16 / 65536 (0 .. 65536); 0 .. 8 masks of each kind.  All zero: the plain copy, bit for bit.
 *   seq_lens  int32 [batch], the utterances' own lengths (0 .. frames; the kernel clamps, the host forms refuse others)
 *   draw_ids  int64 [batch]: with `seed` the whole source of an utterance's randomness (Philox4x32-10, key = seed, counter =
 *             {draw id, block, 0}; which block and word feeds which draw: csrc/spec_augment_core.h).  Nothing depends on the
 *             utterance's row, the batch size, the padded length or the rest of the batch.
 *   plan_out  optional int32 [batch][2 + 2 (freq_masks + time_masks)]: per utterance {c, w, (f0, f) per frequency mask, (t0, t)
 *             per time mask}; the warp maps output row c + w to source row c, c = w = 0 when the utterance is not warped.
 * st_spec_augment_host: the same on HOST pointers (dst->base a host buffer of the same geometry), bit-identical to the kernel: the
 *   two share their arithmetic.  st_spec_augment_plan_host: the plans only (any length >= 0).  Neither needs a GPU. */
int st_spec_augment_f32(const float* src, int batch, int frames, int channels, const int32_t* seq_lens, const int64_t* draw_ids,
                        uint64_t seed, int time_warp, int freq_width, int freq_masks, int time_width, int time_masks,
                        int time_ratio_q16, const st_tensor3* dst, int32_t* plan_out, void* stream);
int st_spec_augment_host(const float* host_src, int batch, int frames, int channels, const int32_t* host_seq_lens,
                         const int64_t* host_draw_ids, uint64_t seed, int time_warp, int freq_width, int freq_masks, int time_width,
                         int time_masks, int time_ratio_q16, const st_tensor3* host_dst, int32_t* host_plan_out);
int st_spec_augment_plan_host(const int32_t* host_seq_lens, const int64_t* host_draw_ids, int batch, int channels, uint64_t seed,
                              int time_warp, int freq_width, int freq_masks, int time_width, int time_masks, int time_ratio_q16,
                              int32_t* host_plan_out);

/* ---- Waveform augmentation before the features (csrc/wave_augment.hip, csrc/wave_augment_core.h; no reference counterpart).  A
 * batch of utterances stored one after the other (fp32; utterance u = in[in_offsets[u] .. in_offsets[u + 1])) is written to
 * out[out_offsets[u] ..), each resampled by the speed its plan names and, when its plan says so, mixed with a clip of a noise bank at
 * the planned signal-to-noise ratio.  The full definition (time map, tap order, the fixed order of the power sums, the draws) is at
 * the top of csrc/wave_augment_core.h.
 *   speeds    HOST int32 [n_speeds][2] = {num, den}: reduced fractions, terms 1 .. 32, 1/2 <= num/den <= 2; 1 .. 8 of them.  An
 *             utterance of n samples at num/den becomes M = ceil(n den / num) samples; 1/1 is the copy, bit for bit.
 *   tables    fp32, the speeds' phase tables one after the other, [den][2H] each with H = ceil(16 max(1, num/den)) (one of 1/1 is
 *             present and never read).  The caller makes them (speecht_amd.augmentation.speed_table: resampy's kaiser_fast window,
 *             rows normalised in float64): y[m] = sum_k fmaf(h[phi][k], x[i - H + 1 + k]) in float32, k ascending.
 *   noise     fp32 clips one after the other, clip k = noise[clip_offsets[k] .. clip_offsets[k + 1]) (int64 [n_clips + 1], each clip
 *             1 .. 2^31 - 1 samples), read circularly from the planned offset.  n_clips = 0: no bank, nothing is mixed.
 *   plan      one 40-byte record per utterance, made by st_wave_augment_plan_host and uploaded by the caller:
 *             {int64 M, int64 offset, double lin = 10^(snr/10), int32 speed index (-1: 1/1), int32 noisy, int32 clip, int32 snr in
 *             hundredths of a dB}.  Gain a = sqrt(Ps / (Pn lin)) in double from the two mean powers over the M outputs (0 when
 *             either is 0, and then nothing is mixed); out[m] = fmaf((float)a, noise sample, resampled sample).
 * st_wave_augment_plan_host: the plans of n_utts utterances of `lengths` samples (0 .. 2^30 - 1), no GPU needed.  Draws are Philox4x32-10
 *   with key = seed and counter = {draw id, block, 1} (SpecAugment's counter ends in 0: the two never share a stream), a function of
 *   (seed, draw id) alone.  noise_prob_q16 in 0 .. 65536; the SNR is uniform over snr_lo_centi .. snr_hi_centi hundredths of a dB.  A
 *   drawn speed that would leave M <= min_samples is replaced by 1/1 (speed index -1).
 * st_wave_augment_f32: DEVICE pointers except `speeds`; two launches on `stream` (the second only with a bank).  in_total / out_total:
 *   floats of `in` / `out`; max_out: the largest planned M (the caller knows every M from the plan).  The plan is device memory, so
 *   the kernels clamp whatever it says to the offsets tables and the totals before they address anything.  Workspace (the tile
 *   sums, needed with a bank): st_wave_augment_ws(n_utts, max_out) bytes, 8-byte aligned; any content.
 * st_wave_augment_host: the same on HOST pointers, bit-identical to the kernels (the two share their arithmetic), every plan entry
 *   checked.  sums_out: optional double [n_utts][2], the two sums of squares of each noisy utterance (0 otherwise).  No GPU needed. */
int st_wave_augment_plan_host(const int64_t* host_lengths, const int64_t* host_draw_ids, int n_utts, uint64_t seed,
                              const int32_t* host_speeds, int n_speeds, int noise_prob_q16, int snr_lo_centi, int snr_hi_centi,
                              const int64_t* host_clip_lens, int n_clips, int64_t min_samples, void* host_plan_out);
size_t st_wave_augment_ws(int n_utts, int64_t max_out);
int st_wave_augment_f32(const float* in, const int64_t* in_offsets, int n_utts, int64_t in_total, const void* plan,
                        const int32_t* host_speeds, int n_speeds, const float* tables, const float* noise, const int64_t* clip_offsets,
                        int n_clips, float* out, const int64_t* out_offsets, int64_t out_total, int64_t max_out, void* workspace,
                        size_t workspace_bytes, void* stream);
int st_wave_augment_host(const float* host_in, const int64_t* host_in_offsets, int n_utts, const void* host_plan,
                         const int32_t* host_speeds, int n_speeds, const float* host_tables, const float* host_noise,
                         const int64_t* host_clip_offsets, int n_clips, float* host_out, const int64_t* host_out_offsets,
                         double* host_sums_out);

/* ---- helpers -------------------------------------------------------------------------- */
int st_fill_f32(float* dst, float value, size_t n, void* stream);
/* zero the halo rows of a padded NWC tensor (needed when a buffer is re-described for a new shape) */
int st_zero_halos_f32(const st_tensor3* t, void* stream);
/* ... and the same for every buffer of a shape in ONE launch: `regions_device` is a DEVICE table of n_regions pairs
 * {uint64 address, uint64 bytes} (addresses and sizes multiples of 16; one workgroup zeroes one range, so long ranges are best cut
 * into pieces of ~1 MB).  The engine keeps one table per (batch, frames) shape it has seen: re-entering a shape -- the reference pads
 * every batch to its own longest member (speech_input.py:37-45), so that is nearly every step -- costs one launch, not one per tensor. */
int st_zero_regions(const void* regions_device, int n_regions, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SPEECHT_HIP_H */
