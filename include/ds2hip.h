/* ds2hip.h -- C ABI of libds2hip.so: MI355X (gfx950) kernels for the DeepSpeech2 train-step hot path.
 *
 * The reference (SeanNaren/deepspeech.pytorch) is pure Python and has NO FFI/plugin interface: its boundary for this
 * path is the Python class deepspeech_pytorch.model.DeepSpeech (model.py:138-310).  This header is the C-ABI seam
 * placed directly beneath that class: one entry per stage of DeepSpeech.forward / training_step, each citing the
 * reference lines it replaces.  A maintainer binds it with ctypes; the shipped binding is
 * deepspeech/pytorch_amd/_lib.py and the drop-in class is deepspeech/pytorch_amd/model.py.
 *
 * Conventions
 *  - Every pointer is a DEVICE pointer unless named *_host.  The library never allocates or frees device memory and
 *    never synchronises: the caller owns all buffers (torch's caching allocator) and passes the stream (a hipStream_t) to launch
 *    on (torch.cuda.current_stream().cuda_stream).  Re-entrant, no thread-local state (backward runs on autograd's
 *    worker thread).
 *  - Return value: 0 = ok; >0 = hipError_t of a failed launch; DS2_ERR_* (>= 1000) = argument errors.
 *  - dtype selects the activation STORAGE type (and the MFMA operand type): DS2_F32 or DS2_BF16 (raw uint16 bits).
 *    Accumulation, statistics, gate math, CTC and all parameter gradients are fp32.
 *  - "T" below means the storage type selected by dtype.
 *  - Activation layouts (internal to this library; only the class boundary must match the reference):
 *      conv activations   NFTC : [N][F][T'][32]   (channel fastest)                 reference: NCHW (N,32,F,T')
 *      sequence matrices  rows = t*N + n, features fastest: [T'*N][ld]              reference: (T',N,H)
 *      conv->RNN features are ordered f*32+c (reference model.py:219-221 orders c*41+f; the binding permutes the
 *      columns of rnns.0 weight_ih accordingly, parameters themselves keep the reference layout).
 */
#ifndef DS2HIP_H
#define DS2HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* a hipStream_t, passed as a plain pointer so that the header needs no HIP headers */
typedef void* ds2_stream_t;

enum { DS2_F32 = 0, DS2_BF16 = 1 };
enum { DS2_CELL_GRU = 0, DS2_CELL_LSTM = 1, DS2_CELL_RNN_TANH = 2 };
enum {
  DS2_OK = 0,
  DS2_ERR_DTYPE = 1001, /* unknown dtype */
  DS2_ERR_ARG = 1002,   /* bad dimension / null pointer / unsupported combination */
  DS2_ERR_ALIGN = 1003  /* pointer or leading dimension not 16-byte aligned / not a multiple of the vector width */
};

int ds2_version(void);
const char* ds2_error_string(int code);

/* ---- dense contraction (MFMA): C[M][ldc] = A[M][lda] * B[N][ldb]^T (+ bias[N]) -------------------------------------
 * Replaces the GEMMs inside torch's GRU/LSTM input projection (model.py:97-99), nn.Linear of the head (model.py:197)
 * and their autograd backward.  out_f32 != 0 -> C is float regardless of dtype.  splitk > 1: C is f32 and is zeroed by the call (memset nodes on `stream`). */
int ds2_gemm_nt(int dtype, const void* A, const void* B, void* C, const float* bias, int M, int N, int K, long lda, long ldb,
                long ldc, int out_f32, int batch, long strideA, long strideB, long strideC, long strideBias, int splitk,
                ds2_stream_t stream);

/* same contract as ds2_gemm_nt; selects the low-register kernel variant whose waves can share a CU with the persistent
 * recurrent kernels (weight-gradient GEMMs issued on a second stream while a sweep runs). */
/* A as two row blocks (rows [0,m_split) from A, the rest from A2, same lda); coresident != 0: the low-register kernel. */
int ds2_gemm_nt_rows2(int dtype, const void* A, const void* A2, int m_split, const void* B, void* C, int M, int N, int K, long lda,
                      long ldb, long ldc, int out_f32, int splitk, int coresident, ds2_stream_t stream);
int ds2_gemm_nt_coresident(int dtype, const void* A, const void* B, void* C, const float* bias, int M, int N, int K, long lda,
                           long ldb, long ldc, int out_f32, int batch, long strideA, long strideB, long strideC, long strideBias,
                           int splitk, ds2_stream_t stream);

/* 256x256-tile bf16 kernel with a phase-split schedule (csrc/ds2_gemm8.hip) for the large contractions of the step.
 * ds2_gemm8_nt: same product as ds2_gemm_nt (bf16 operands; C bf16 or f32); K % 64 == 0, lda/ldb % 8 == 0.  The input
 * projections of torch's GRU/LSTM and the dX products of their backward (model.py:97-99).
 * ds2_gemm8_tn_grouped: n_problems (<= 6) products C_i[M_i][ldc_i] f32 = sum_{k<K} At_i[k][m] * Bt_i[k][n] in ONE launch -- both
 * operands K-major, i.e. stored as the activations are ([T'*N rows][features]): the weight gradients dW_ih = dGI^T X and
 * dW_hh = dGH^T h_prev of the recurrent layers' backward without operand transposes.  At2_i (may be NULL): output rows >=
 * m_split_i (a multiple of 256) take their operand columns from At2_i (column m - m_split_i, leading dimension lda2_i) -- the GRU's hidden-side
 * gate gradient [dr, dz | dQ] lives in two buffers.  Any K (no row past K - 1 is read); M_i, N_i, lda, ldb % 8 == 0. */
int ds2_gemm8_nt(const void* A, const void* B, void* C, const float* bias, int M, int N, int K, long lda, long ldb, long ldc, int out_f32,
                 ds2_stream_t stream);
int ds2_gemm8_tn_grouped(int n_problems, const void* const* At, const void* const* At2, const int* m_split, const void* const* Bt, void* const* C,
                         const int* M, const int* N, const long* lda, const long* lda2, const long* ldb, const long* ldc, int K, ds2_stream_t stream);

/* ds2_gemm8_wgrad_dx: the TN problems of ds2_gemm8_tn_grouped (n_tn <= 5) AND one NT product (bf16 out, no bias; the dX of the
 * layer: same contract as ds2_gemm8_nt) in ONE launch, long tiles first -- the backward of one recurrent layer behind its sweep. */
int ds2_gemm8_wgrad_dx(int n_tn, const void* const* At, const void* const* At2, const int* m_split, const void* const* Bt, void* const* C,
                       const int* M, const int* N, const long* lda, const long* lda2, const long* ldb, const long* ldc, int K_tn,
                       const void* A_nt, const void* B_nt, void* C_nt, int M_nt, int N_nt, int K_nt, long lda_nt, long ldb_nt, long ldc_nt,
                       ds2_stream_t stream);

/* Row lists: the `_rows` forms of the three entries above visit only the listed rows of the dimension that runs over the
 * [T' x batch] frames of a padded sequence matrix -- the frames t < length of every clip, i.e. what pack_padded_sequence keeps
 * (model.py:96; the reference's nn.GRU / nn.LSTM never see the padding, model.py:97-100).  rows: device int32 [n_rows], values in
 * [0, n_phys); null = every row.
 *   ds2_gemm8_nt_rows:          C[rows[r]][:] = A[rows[r]][:] * B^T (+ bias), r < n_rows; the other rows of C are NOT written.
 *   ds2_gemm8_tn_grouped_rows:  C_i = sum over k < n_rows of At_i[rows[k]][m] * Bt_i[rows[k]][n].
 *   ds2_gemm8_wgrad_dx_rows:    both (K_tn == M_nt == n_phys).
 * ds2_zero_pad_rows: X[(t*N + n)][0..cols) = 0 for t >= lens[n] (the rows a `_rows` product leaves unwritten). */
int ds2_gemm8_nt_rows(const void* A, const void* B, void* C, const float* bias, int n_phys, int N, int K, long lda, long ldb, long ldc,
                      int out_f32, const int* rows, int n_rows, ds2_stream_t stream);
int ds2_gemm8_tn_grouped_rows(int n_problems, const void* const* At, const void* const* At2, const int* m_split, const void* const* Bt,
                              void* const* C, const int* M, const int* N, const long* lda, const long* lda2, const long* ldb, const long* ldc,
                              int n_phys, const int* rows, int n_rows, ds2_stream_t stream);
/* Start offsets of an NT launch's first round (csrc/ds2_gemm8.hip, g8_stagger_wait): the workgroups that open the CUs wait
 * id * span / CUs before their first tile, so that the tiles of a CU round do not reach their store epilogues at one moment.
 * Results do not depend on the span.  ds2_gemm8_stagger_plan: the span in microseconds that a launch of `tiles` tiles gets on
 * `cus` CUs -- kind 0 NT (ds2_gemm8_nt, _nt_rows: non-zero only from 2 * cus tiles), 1 grouped TN and 2 mixed (always 0); kind < 0:
 * the longest span an entry accepts.  Host only, no device is asked.  ds2_gemm8_nt_rows_stagger: ds2_gemm8_nt_rows with the span
 * given (stagger_us < 0: the policy's; otherwise clamped to the longest span and applied whatever the tile count). */
int ds2_gemm8_stagger_plan(int kind, int tiles, int cus);
int ds2_gemm8_nt_rows_stagger(const void* A, const void* B, void* C, const float* bias, int n_phys, int N, int K, long lda, long ldb, long ldc,
                              int out_f32, const int* rows, int n_rows, int stagger_us, ds2_stream_t stream);
int ds2_gemm8_wgrad_dx_rows(int n_tn, const void* const* At, const void* const* At2, const int* m_split, const void* const* Bt, void* const* C,
                            const int* M, const int* N, const long* lda, const long* lda2, const long* ldb, const long* ldc, int K_tn,
                            const void* A_nt, const void* B_nt, void* C_nt, int M_nt, int N_nt, int K_nt, long lda_nt, long ldb_nt, long ldc_nt,
                            const int* rows, int n_rows, ds2_stream_t stream);
int ds2_zero_pad_rows(int dtype, void* X, long ld, int cols, const int* lens, int Tp, int N, ds2_stream_t stream);

/* ---- BatchNorm (model.py:159,162 BatchNorm2d in NFTC; model.py:28-33,86,196 SequenceWise BatchNorm1d) ---------------
 * mode 0: sequence matrix X[R][ldx], C features.   mode 1: conv activation NFTC (R = N*F*Tp rows, C = 32): output also
 * gets Hardtanh(0,20) (model.py:160,163) and the MaskConv time mask (model.py:61-68; t >= lens[n] -> 0).
 * mode 2: like 1 but Y (fwd) / G (bwd) are in sequence layout [(t*N+n)][f*32+c] (fuses model.py:219-221).
 * training != 0: batch statistics over ALL rows (biased variance), running stats updated with `momentum` (unbiased
 * variance), num_batches_tracked += 1.  save_* (C floats each) are kept for backward.  ws: 2*ds2_norm_partials(R)*C floats.*/
int ds2_norm_partials(long R);
int ds2_bn_fwd(int dtype, int mode, int training, const void* X, void* Y, long R, int C, long ldx, long ldy, int F, int Tp,
               int N, const int* lens, const float* gamma, const float* beta, float* running_mean, float* running_var,
               long long* num_batches_tracked, float eps, float momentum, float* save_mean, float* save_rstd,
               float* save_scale, float* save_shift, float* ws, ds2_stream_t stream);
/* G = upstream gradient (gated by Hardtanh' and the mask in modes 1/2), X = the forward input of the BN.
 * ws: (2*ds2_norm_partials(R) + 2) * C floats. */
int ds2_bn_bwd(int dtype, int mode, const void* G, const void* X, void* DX, long R, int C, long ldg, long ldx, long lddx,
               int F, int Tp, int N, const int* lens, const float* save_mean, const float* save_rstd,
               const float* save_scale, const float* save_shift, float* dgamma, float* dbeta, float* ws,
               ds2_stream_t stream);
/* out[c] = scale * sum_r X[r][c]  (bias gradients; ws: ds2_norm_partials(R)*C floats) */
int ds2_colsum(int dtype, const void* X, long R, int C, long ld, float* out, float scale, float* ws, ds2_stream_t stream);

/* ---- conv front-end (MaskConv over model.py:157-164) ------------------------------------------------------------------
 * F0 = input frequency bins = sample_rate * window_size / 2 + 1 (model.py:166: 161 at 16 kHz / 20 ms, 81 at 8 kHz); F1, F2 = rows
 *      after the two convolutions (model.py:167-168; ds2_conv_rows: 161 -> 81 -> 41).  The bf16 matrix-pipe kernels are specialised
 *      for 161 bins; every other geometry runs the general kernels of the same storage type.
 * conv1: Conv2d(1,32,(41,11),stride (2,2),pad (20,5)) on x (N,1,F0,T) f32 -> y1 NFTC [N][F1][Tp][32] (T), bias added,
 *        time mask applied.  w1k = weight re-laid as [41*11][32] f32 (tap-major, out-channel fastest).
 * conv2: Conv2d(32,32,(21,11),stride (2,1),pad (10,5)) on a1 NFTC [N][F1][Tp][32] -> y2 NFTC [N][F2][Tp][32];
 *        w2t = weight re-laid as [21*11][32 out][32 in] (T).
 * dgrad: da1 = conv2^T(dy2) with w2d = the two stride-parity sub-kernels, layout documented in _lib.py/prep. */
int ds2_conv_rows(int F0, int* F1, int* F2);
int ds2_conv1_fwd(int dtype, const float* x, const float* w1k, const float* b1, const int* lens, void* y1, int N, int F0, int T,
                  int Tp, ds2_stream_t stream);
/* dw1k [451][32] f32 = sum over positions of dy1 (NFTC, T) x input taps.  ws: ds2_conv1_wgrad_ws_floats(N,F0,Tp) floats. */
long ds2_conv1_wgrad_ws_floats(int N, int F0, int Tp);
int ds2_conv1_wgrad(int dtype, const float* x, const void* dy1, float* dw1k, int N, int F0, int T, int Tp, float* ws,
                    ds2_stream_t stream);
/* ws: ds2_conv2_fwd_ws_bytes(dtype,N,F0,Tp) bytes (bf16 storage at 161 bins: fp32 partial sums of the even-kernel-row half of the
 * layer pass through it; 0 and ws may be NULL otherwise). */
long ds2_conv2_fwd_ws_bytes(int dtype, int N, int F0, int Tp);
int ds2_conv2_fwd(int dtype, const void* a1, const void* w2t, const float* b2, const int* lens, void* y2, int N, int F0, int Tp,
                  void* ws, ds2_stream_t stream);
int ds2_conv2_dgrad(int dtype, const void* dy2, const void* w2d_even, const void* w2d_odd, void* da1, int N, int F0, int Tp,
                    ds2_stream_t stream);
/* dw2t [231][32 out][32 in] f32.  ws: ds2_conv2_wgrad_ws_floats(N,Tp) floats. */
long ds2_conv2_wgrad_ws_floats(int N, int Tp);
int ds2_conv2_wgrad(int dtype, const void* dy2, const void* a1, float* dw2t, int N, int F0, int Tp, float* ws, ds2_stream_t stream);

/* ---- recurrent sweeps (BatchRNN, model.py:94-102; nn.GRU / nn.LSTM / nn.RNN(tanh), enums.py:17-21) ---------------------
 * See csrc/ds2_rnn.hip for the buffer shapes.  H % 16 == 0. */
int ds2_rnn_gates(int cell);
int ds2_rnn_saved_planes(int cell);
long ds2_rnn_state_bytes(int D, int N, int H);
int ds2_rnn_fwd(int dtype, int cell, int D, int N, int H, int Tp, const int* lens, const void* GI, const void* Whh,
                const float* bhh, const float* h0, const float* c0, void* Hseq, long hseq_dstride, void* S, float* hn, float* cn,
                void* state, ds2_stream_t stream);
/* h0 / c0 [D][N][H] f32 (may be NULL = zeros): the initial state the forward was given (`hs`, model.py:224-230); dh0 / dc0 (may be
 * NULL): d loss / d h0, d c0.  Only the launch-per-time-step BPTT takes them (training through a given `hs` is the rare path; the
 * persistent sweeps assume a zero initial state in backward). */
int ds2_rnn_bwd(int dtype, int cell, int D, int N, int H, int Tp, const int* lens, const void* dOut, const void* WhhT,
                const void* Hseq, long hseq_dstride, const void* S, void* dGI, void* dGH, const float* h0, const float* c0,
                float* dh0, float* dc0, void* state, ds2_stream_t stream);

/* Persistent variant (csrc/ds2_rnn_persist.hip): one launch per sweep, all time steps inside the kernel, W_hh resident in
 * registers, h exchanged between the workgroups of a group through a polled exchange buffer inside ws (pure payload in four
 * slots with an all-ones "not published yet" dword, or tagged 8-byte granules: csrc/ds2_rnn_persist_impl.h); same buffer contract as
 * ds2_rnn_fwd / ds2_rnn_bwd.  Covered (ds2_rnn_persist_supported): bf16 with H = 1024 (any cell, <= 16 samples per group of an
 * 8-group chip: BASELINE config 3); GRU / LSTM with bf16 storage at the widths of DS2_PERSIST3_WIDTHS and <= 32 samples per group
 * (round-4 general kernels: 32 units per workgroup, groups inside one XCD for H <= 1024 -- config 5); the (cell, type, H, m-tiles)
 * rows of DS2_PERSIST2_INSTANCES with <= 64 samples per group (round-2 general kernels: config 2, the 1e-3 parity mode) -- both
 * tables are csrc/ds2_rnn_persist_widths.h, the one list of instantiated widths; everything else runs ds2_rnn_fwd / _bwd.
 * ws: ds2_rnn_persist_ws_bytes() bytes of scratch (reset by every call on `stream`); err: one device int, sticky (maximum): 1 = a
 * workgroup gave up waiting for its peers in the middle of a sweep, 2 = the launch's workgroups never became co-resident within
 * opts->startup_ms; the outputs are then NaN-poisoned. */
/* Per-launch options of the persistent sweeps; pass NULL for the defaults.  (Rounds 2-5 had process-wide setters here --
 * ds2_rnn_persist_set_variant / _set_spin_limit; options travel with the call now: the entries are re-entrant, backward may run on
 * autograd's worker thread beside a forward, and nothing a caller sets outlives its call.)
 *   variant     routing bits for tests and measurements, 0 = the shipping routing.  Three bits are live: bit 0 (1) the shapes of the
 *               round-4 general kernels (csrc/ds2_rnn_persist3_impl.h) run on the round-2 general kernels (or one launch per time
 *               step) instead, bit 3 (8) the round-4 kernels also take H = 1024, bit 4 (16) the tuned kernels keep 9-16 clips per
 *               group.  Any other bit is refused: ds2_rnn_persist_plan / _supported / _kind / _ws_bytes answer 0 and the sweeps
 *               return DS2_ERR_ARG.  (Bits 1, 5, 6 and 7 selected rejected A/B paths; removed, last present in 099aa25.)
 *               The queries below take the same bits, so that a caller sizes the scratch for the routing it will launch.
 *   spin_limit  fault injection: polls a workgroup may spend on ONE mid-sweep exchange wait before it gives up (raises *err = 1,
 *               NaN-poisons its outputs, ends); 0 = the built-in budget (~seconds).
 *   startup_ms  how long (wall clock) the workgroups of a launch wait for ALL of them to become resident before the first exchange;
 *               a sweep needs every workgroup on a CU of its own at the same time, so a kernel of another process -- or an RCCL
 *               collective on another stream that waits for a late peer rank -- keeps it from starting.  0 = 300 ms: right for a
 *               single process (nothing legitimate holds CUs that long; *err = 2 names the cause).  Under data parallelism pass
 *               the process group's time-out: a sweep behind a collective must wait, as any stock kernel would simply queue
 *               (configs/librispeech.yaml:14 `strategy: ddp`; loader/data_loader.py:320-360 hands ranks unequal batches). */
typedef struct ds2_persist_opts {
  unsigned variant;
  unsigned spin_limit;
  unsigned startup_ms;
} ds2_persist_opts;
/* The routing decision behind every entry below, with the CU count given instead of asked of the current device (256 = a full
 * MI355X): returns the kernel family (ds2_rnn_persist_kind's numbers) and stores the scratch bytes of one sweep in *ws_bytes (may be
 * NULL; 0 for family 0).  Host arithmetic only -- no device is needed, so the routing table can be pinned by a host test. */
int ds2_rnn_persist_plan(int dtype, int cell, int D, int N, int H, int cus, unsigned variant, long* ws_bytes);
int ds2_rnn_persist_supported(int dtype, int cell, int D, int N, int H, unsigned variant);
/* 1 if a persistent kernel exists for the problem on a FULL device (256 CUs), whatever the current device exposes: tells "this
 * device is too small for the persistent sweeps" (the caller raises) from "no persistent kernel for this shape" (it warns). */
int ds2_rnn_persist_shape_covered(int dtype, int cell, int D, int N, int H);
/* Kernel family the persistent entries run for the problem on the current device: 0 none (ds2_rnn_fwd / _bwd), 1 / 2 tuned H = 1024
 * (<= 8 / 9-16 samples per group), 3 round-4 general (k_rnn_persist3_*), 4 round-2 general (k_rnn_persist2_*). */
int ds2_rnn_persist_kind(int dtype, int cell, int D, int N, int H, unsigned variant);
long ds2_rnn_persist_ws_bytes(int dtype, int cell, int D, int N, int H, unsigned variant);
int ds2_rnn_persist_fwd(int dtype, int cell, int D, int N, int H, int Tp, const int* lens, const void* GI, const void* Whh,
                        const float* bhh, const float* h0, const float* c0, void* Hseq, long hseq_dstride, void* S, float* hn,
                        float* cn, void* ws, int* err, const ds2_persist_opts* opts, ds2_stream_t stream);
/* BPTT: dGI as ds2_rnn_bwd; GRU: dQ [D][Tp][N][H] = dn*r (the one slot of the hidden-side gate gradient [dr,dz,dQ] that differs
 * from dGI's; null for LSTM / RNN); dBacc [D][N][NB*H] f32 (may be null): per-sample sums over time of the stored gate-gradient
 * planes (NB = 4 for GRU: dr, dz, dn, dQ; G otherwise) -- the bias gradients are their sums over the samples. */
/* flags bit 0: the caller never reads the padding rows (t >= lens[n]) of dGI / dQ -- its products over the frames run on a row list
 * (ds2_gemm8_*_rows) and its bias gradients come from dBacc -- so a sweep whose half-steps leave those rows unwritten (two-set groups
 * of the round-4 general kernels) skips zeroing them. */
int ds2_rnn_persist_bwd(int dtype, int cell, int D, int N, int H, int Tp, const int* lens, const void* dOut, const void* WhhT,
                        const void* Hseq, long hseq_dstride, const void* S, void* dGI, void* dQ, float* dBacc, int flags, void* ws,
                        int* err, const ds2_persist_opts* opts, ds2_stream_t stream);

/* ---- small sequence ops ---------------------------------------------------------------------------------------------------
 * add2: out = a + b (direction sum, model.py:101).  transpose: dst[C][ldd] = src[R][lds]^T, zero-filling r in [R, ldd).
 * lookahead (model.py:105-135, uni-directional models): y[t] = hardtanh(sum_k w[h][k] * x[t+k]), x/y [Tp*N][H] (T),
 * w [H][ctx] f32, any ctx >= 1 (ctx = 20, the reference default, takes the sliding-window kernels: one load per operand and frame);
 * `pre` keeps the pre-Hardtanh value for backward (may be null in eval).
 * bwd: dx and dw (dw via ws of ds2_lookahead_ws_floats). */
int ds2_add2(int dtype, const void* a, const void* b, void* out, long n, ds2_stream_t stream);
/* out[n] f32 = the sum of `slices` consecutive [n] blocks of src, added in index order: the fixed-order reduction of a product whose
 * contraction was cut into K-slices (ds2_gemm_nt with the slices as its batch) -- the fp32-mode dX of nn.GRU / nn.LSTM (model.py:97-99
 * backward: few output tiles, long K) without the run-to-run summation order of atomic split-K.  n % 4 == 0. */
int ds2_sum_slices(const float* src, float* out, long n, int slices, ds2_stream_t stream);
int ds2_transpose(int dtype, const void* src, void* dst, long R, int C, long lds, long ldd, ds2_stream_t stream);
/* fp32 operand [rows][K] (row stride lds) -> bf16 [rows][3 * Kp] (row stride ldd; Kp = K rounded up to 64, zero beyond K): the K
 * segments [hi | hi | lo] (mode 0, the A operand of a product) or [hi | lo | hi] (mode 1, the B operand) with hi = bf16(x),
 * lo = bf16(x - hi).  One bf16 GEMM over K' = 3 Kp of two such operands = a_hi b_hi + a_hi b_lo + a_lo b_hi: the fp32-mode (1e-3
 * parity) input projections / dX / weight gradients of nn.GRU / nn.LSTM (model.py:97-99) on the bf16 matrix pipe.
 * Modes 2 / 3 (round 6): the same three segments stacked by ROWS -- dst [3 * rows][ldd], segment s at row s * rows, Kp = K rounded up
 * to 8 -- i.e. the operands of a TN product (ds2_gemm8_tn_grouped: the contraction index is the row), so that the fp32-mode weight
 * gradients run over the activations as stored, without operand transposes. */
int ds2_split3_bf16(const float* src, long lds, long rows, int K, int Kp, int mode, void* dst, long ldd, ds2_stream_t stream);
/* Weight re-layout of the recurrent layers (what nn.GRU/LSTM/RNN.flatten_parameters + the autocast weight casts do in the
 * reference, model.py:97-99): fp32 src[R][C] -> bf16 dst[R][ldd] and/or bf16 transpose dstT[Cout][lddT] in one pass.
 * perm_c > 0: output column j = f*perm_c + c takes source column c*perm_f + f (rnns.0 reads the conv features in the
 * kernels' [f][c] order; the reference flattens [c][f], model.py:219-220); columns [C, Cout) are zero.  R % 16 == 0. */
int ds2_cast_transpose_bf16(const float* src, long lds, int R, int C, int perm_c, int perm_f, int Cout, void* dst, long ldd,
                            void* dstT, long lddT, ds2_stream_t stream);
/* Kernel layouts of the small weights in one launch (the per-step re-layout of conv.seq_module.{0,3}.weight and fc weight after
 * the optimizer step; model.py:158,161,197): w1k [451][32] f32 = conv1 weight tap-major; w2t [21][11][co][ci] (T) conv2 forward;
 * w2d0 [11][11][ci][co] / w2d1 [10][11][ci][co] (T) = the flipped even / odd kernel-row sub-kernels of the conv2 data gradient;
 * wfcp [32][H] (T) = head weight zero-padded to 32 classes, wfcT [H][32] (T) its transpose.
 * ds2_scale_by: x[i] *= *s (s on the device) -- the upstream gradient of the summed CTC loss. */
int ds2_small_weight_layouts(int dtype, const float* w1, const float* w2, const float* wfc, int C, int H, float* w1k, void* w2t,
                             void* w2d0, void* w2d1, void* wfcp, void* wfcT, ds2_stream_t stream);
int ds2_scale_by(float* x, const float* s, long n, ds2_stream_t stream);

/* ds2_copy_words: dst[0..n_words) = src[0..n_words) (4-byte words), as a kernel on `stream`.  Either pointer may be pinned
 * (device-mapped) host memory.  Replaces the reference's implicit host->device transfers of the per-step index tables -- the
 * lengths `.cpu()` / BoolTensor masks `.cuda()` of MaskConv (model.py:61-68,215) and the CTC target table (model.py:248) -- and the
 * device->host read of the persistent sweeps' error word: hipMemcpyAsync would hand these to the SDMA engines, whose transfers run
 * under the kernels of earlier steps when the host thread is ahead and cost a latency-bound sweep 1-2 ms each. */
int ds2_copy_words(const void* src, void* dst, long n_words, ds2_stream_t stream);
int ds2_lookahead_fwd(int dtype, const void* x, const float* w, void* y, void* pre, int Tp, int N, int H, int ctx,
                      ds2_stream_t stream);
long ds2_lookahead_ws_floats(int Tp, int N, int H, int ctx);
int ds2_lookahead_bwd(int dtype, const void* x, const float* w, const void* pre, const void* dy, void* dx, float* dw, int Tp,
                      int N, int H, int ctx, float* ws, ds2_stream_t stream);
/* bias_ih.grad [D][G*H] and bias_hh.grad [D][G*H] of a recurrent layer (torch GRU/LSTM/RNN backward, model.py:97-99) from the
 * per-sample sums dBacc [D][N][NB*H] that ds2_rnn_persist_bwd accumulates (cell: 0 GRU, 1 LSTM, 2 tanh RNN). */
int ds2_rnn_bias_grads(int cell, int D, int N, int H, const float* dBacc, float* dbih, float* dbhh, ds2_stream_t stream);

/* ---- output layer for at most 64 padded classes (model.py:195-201, Linear(H, C, bias=False)) --------------------------------------
 * Xh [R][ldx] bf16 (H columns used), Wp [Cp][ldw] bf16 = the head weight zero-padded to Cp = 32 or 64 classes, H % 8 == 0.  Both
 * passes are bound by the activation matrix and move it once, in 16-byte pieces; products on the bf16 matrix pipe, fp32 accumulation
 * in a fixed order (the same bits in every run).  ds2_fc_supported: 1 for the (H, Cp) these entries take (Wp must fit the forward's
 * LDS image: Cp * H <= 64 Ki elements), else the caller keeps ds2_gemm_nt.
 * fwd: logits [R][ldl] f32 = Xh * Wp^T.
 * bwd: dXh [R][lddx] bf16 = bf16(dlogits) * Wp and dW [Cp][H] f32 = bf16(dlogits)^T * Xh from dlogits [R][ldg] f32 and Xh as stored
 * (no cast pass, no transposes; Xh is read once): the fp32 partials of dW over row blocks of block_rows rows (a multiple of 32;
 * ds2_fc_bwd_partials(R, block_rows) of them) go to ws (that many * Cp * H floats) and a last launch adds them in index order: no
 * atomics.  The three products keep the 16-wide k-steps, their order and the operand slots of ds2_gemm_nt: with block_rows = the
 * slice length of a K-sliced ds2_gemm_nt (+ ds2_sum_slices) over the same rows, the results have that path's bits. */
int ds2_fc_supported(int H, int Cp);
int ds2_fc_fwd(const void* Xh, long ldx, const void* Wp, long ldw, float* logits, long ldl, long R, int H, int Cp, ds2_stream_t stream);
long ds2_fc_bwd_partials(long R, long block_rows);
int ds2_fc_bwd(const float* dlogits, long ldg, const void* Xh, long ldx, const void* Wp, long ldw, void* dXh, long lddx, float* dW,
               float* ws, long R, int H, int Cp, long block_rows, ds2_stream_t stream);

/* probs = softmax(logits) row-wise (InferenceBatchSoftmax, model.py:72-77), f32 [rows][C] */
int ds2_softmax_rows(const float* logits, float* probs, long rows, int C, long ld_in, long ld_out, ds2_stream_t stream);

/* ---- log_softmax + CTC loss + gradient (model.py:246,203,248) -----------------------------------------------------------
 * logits [Tp*N][ldl] f32 (row = t*N+n, C classes), targets int32 concatenated with target_offsets[N] (start of each
 * sample's labels), input_lengths/target_lengths int32 [N].  blank index `blank`; reduction 'sum'; zero_infinity: an
 * infeasible sample contributes loss 0 and gradient 0.  Outputs: nll [N] f32 (per-sample), loss_sum [1] f32,
 * dlogits [Tp*N][ldg] f32 = grad_scale * d(loss_sum)/d(logits) (log_softmax backward fused; zero rows for t >= length;
 * columns >= C are zero-filled up to ldg).  ws: ds2_ctc_ws_floats(...) floats.  max_target_len: max over target_lengths.
 * recursion: which recursion kernel runs (bit-identical results; for A/B runs and tests): 0 = the default choice (the pair-tile
 * kernel for targets of up to 783 labels, the four-wave kernel beyond), 1 = always the four-wave kernel, 2 = the one-wave kernel up to
 * 255 labels (<= 32 classes), 3 = the choice of rounds 3-5 (one wave up to 63 labels, four waves beyond). */
long ds2_ctc_ws_floats(int Tp, int N, int C, int max_target_len);
int ds2_ctc_loss_grad(const float* logits, long ldl, const int* targets, const int* target_offsets, const int* input_lengths,
                      const int* target_lengths, int Tp, int N, int C, int blank, int max_target_len, float grad_scale,
                      float* nll, float* loss_sum, float* dlogits, long ldg, float* ws, int recursion, ds2_stream_t stream);

/* ---- multi-hypothesis CTC: several label rows per clip against the same frames, one gradient (mwer.py) ------------------------
 * R rows per clip, P = R * N rows in all, rank-major: row p = r * N + n belongs to clip n = p % N (ds2_error_counts' convention).
 * logits, input_lengths [N], blank as for ds2_ctc_loss_grad; targets is the flat int32 label array with target_offsets[P] and
 * target_lengths[P] (a padded [R][N][ld] buffer is target_offsets[p] = p * ld).  A row with target_lengths[p] < 0 is absent; one
 * longer than max_target_len is treated as absent.
 * ds2_ctc_multi_forward: the log-softmax once per clip, then the alpha recursion of every row (grid clip x direction x rank);
 * with want_grad also beta, and the rows stay in ws for ds2_ctc_multi_backward.  nll[p] = -log p(y_p | x_n); +inf for an absent
 * row, an infeasible row and a clip without frames (NOT zero_infinity's 0: the caller's softmax over a clip's rows needs the +inf).
 * want_grad = 0 gives the same nll bits.  recursion: 0 = the pair-tile kernel (the four-wave kernel beyond 783 labels), 1 = always
 * the four-wave kernel; same bits.  R = 1 gives ds2_ctc_loss_grad's nll bits.
 * ds2_ctc_multi_backward: dlogits[t*N + n][:] = sum over the rows p of clip n, in increasing r, of weights[p] * d nll_p / d logits
 * (log-softmax backward fused).  Rows whose nll is +inf contribute nothing whatever their weight (NaN and infinite weights
 * included: they are not read).  Every row of dlogits is written: frames past a clip's length and columns C .. ldg are zero.  The
 * order of additions is fixed: every launch gives the same bits, and R = 1 with weight 1 gives ds2_ctc_loss_grad(grad_scale = 1)'s.
 * It takes the arguments ds2_ctc_multi_forward(want_grad = 1) was called with and its ws.
 * ws: ds2_ctc_multi_ws_floats(...) floats, 8-byte aligned (-1 for arguments the entries refuse): [N][Tp][CP] log-probs, P (rounded
 * up to even) row log-likelihoods, and with want_grad 2 * (P * Tp * (2 max_target_len + 2) + 1) floats of alpha / beta rows. */
long ds2_ctc_multi_ws_floats(int Tp, int N, int R, int C, int max_target_len, int want_grad);
int ds2_ctc_multi_forward(const float* logits, long ldl, const int* targets, const int* target_offsets, const int* target_lengths,
                          const int* input_lengths, int Tp, int N, int R, int C, int blank, int max_target_len, int want_grad,
                          float* nll, float* ws, int recursion, ds2_stream_t stream);
int ds2_ctc_multi_backward(const int* targets, const int* target_offsets, const int* target_lengths, const int* input_lengths, int Tp,
                           int N, int R, int C, int blank, int max_target_len, const float* weights, float* dlogits, long ldg,
                           float* ws, ds2_stream_t stream);

/* ---- MWER weights: the expected error count over an n-best list and its derivative by the rows' nll (ds2_mwer.hip) ------------
 * nll [P] f32 of ds2_ctc_multi_forward, P = (K + has_ref) * N rank-major: ranks 0 .. K-1 are hypotheses, rank K (iff has_ref) the
 * reference.  err [K*N] int32: the error count of every hypothesis (ds2_error_counts), negative = not counted.  Per clip, in fp64
 * with every output rounded to fp32 once: A = the ranks k < K with finite nll and err >= 0; s_k = -nll_k;
 * phat_k = exp(s_k - max_A s) / sum_A exp(s_j - max_A s); ebar = sum_A phat_k err_k; risk[n] = ebar (0 when A is empty);
 * weights[k*N + n] = -phat_k (err_k - ebar) = d risk / d nll_k (0 outside A); weights[K*N + n] = ce_weight when the reference's nll
 * is finite, else 0, and nll_ref[n] = that nll or 0 (zero_infinity).  The reference never joins the softmax.
 * loss[0] = sum_n risk[n] + ce_weight * sum_n nll_ref[n], added in index order.  K = 0 needs has_ref; ce_weight >= 0 and finite. */
int ds2_mwer_weights(const float* nll, const int* err, int N, int K, int has_ref, float ce_weight, float* weights, float* risk,
                     float* nll_ref, float* loss, ds2_stream_t stream);

/* ---- optimizer step (configure_optimizers, model.py:273-297; Lightning's gradient_clip_val, configs/an4.yaml:12) -----------
 * ds2_clip_coef: out[0] = global L2 norm of `count` fp32 gradient tensors, out[1] = min(1, max_norm / (norm + 1e-6)) -- the
 * coefficient torch.nn.utils.clip_grad_norm_ multiplies the gradients by; computed on the device, deterministic order.
 * ds2_opt_multi / ds2_opt_matrix: mode 0 = AdamW, 1 = SGD with Nesterov momentum, fp32, torch's single-tensor arithmetic;
 * hp[7] = {AdamW: 1-lr*wd, 1-beta1, beta2, 1-beta2, sqrt(1-beta2^t), eps, -lr/(1-beta1^t) | SGD: wd, momentum, 0, 0, 1, 0, -lr};
 * first = 1 on SGD's first step; clip = out of ds2_clip_coef (device) or null; v is ignored for SGD.  ds2_opt_matrix also
 * writes the bf16 copy / transpose of the updated matrix (same layout parameters as ds2_cast_transpose_bf16). */
int ds2_opt_max_tensors(void);
long ds2_clip_ws_floats(int count, const long* n);
int ds2_clip_coef(int count, const float* const* g, const long* n, float max_norm, float* out, float* ws, ds2_stream_t stream);
int ds2_opt_multi(int mode, int count, float* const* p, const float* const* g, float* const* m, float* const* v, const long* n,
                  const float* hp, int first, const float* clip, ds2_stream_t stream);
int ds2_opt_matrix(int mode, float* p, const float* g, float* m, float* v, int R, int C, int perm_c, int perm_f, int Cout,
                   void* dst, long ldd, void* dstT, long lddT, const float* hp, int first, const float* clip, ds2_stream_t stream);
/* The kernel ds2_opt_matrix takes for these arguments, host only (the pointers are looked at for null and alignment, never
 * dereferenced): 0 the vectorised k_opt_matrix4 (no permutation, Cout == C, C % 4 == 0, 16-byte aligned operands, ldd % 4 == 0),
 * 1 k_opt_matrix_perm_rows (permutation with perm_c % 8 == 0 and C % 8 == 0, an LDS image of at most 64 KB, aligned operands,
 * ldd % 8 == 0), 2 k_opt_matrix_perm (any other permutation with C % 4 == 0 and aligned fp32 operands), 3 the general k_opt_matrix;
 * arguments ds2_opt_matrix rejects: minus its error code.  ds2_opt_matrix and ds2_opt_matrices both decide through it. */
int ds2_opt_matrix_route(int mode, const void* p, const void* g, const void* m, const void* v, int R, int C, int perm_c, int perm_f,
                         int Cout, const void* dst, long ldd, const void* dstT, long lddT);
/* ds2_opt_matrix for `count` matrices of ONE parameter group (arrays of the per-matrix arguments): every matrix of route 0 (no
 * column permutation, Cout == C, C % 4 == 0, 16-byte aligned) is updated in one launch per 36 of them, the others one by one. */
int ds2_opt_matrices(int mode, int count, float* const* p, const float* const* g, float* const* m, float* const* v, const int* R,
                     const int* C, const int* perm_c, const int* perm_f, const int* Cout, void* const* dst, const long* ldd,
                     void* const* dstT, const long* lddT, const float* hp, int first, const float* clip, ds2_stream_t stream);

/* ---- log-spectrogram front-end (SpectrogramParser.compute_spectrogram, loader/data_loader.py:73-94, + the padded batch layout
 * of _collate_fn, :247-270).  wav [N][ldw] f32 waveforms (utterance n = first nsamples[n] entries of row n; nsamples on the
 * device), n_fft 320 / hop 160 / center = True; basis [322][320] f32 = window-weighted cos rows then -sin rows; reflect: 0 zero
 * centre padding (librosa >= 0.10), 1 reflection; normalize: (x - mean) / unbiased std per utterance.  out (N,1,161,Tmax) f32,
 * Tmax = ds2_spect_frames(Lmax) = 1 + Lmax/160, zero beyond an utterance's own frames.  ws: ds2_spect_ws_bytes(N, Lmax). */
int ds2_spect_frames(int nsamples);
long ds2_spect_ws_bytes(int N, int Lmax);
int ds2_spectrogram(const float* wav, long ldw, const int* nsamples, int N, int Lmax, const float* basis, int reflect,
                    int normalize, float* out, void* ws, ds2_stream_t stream);

/* ---- SpecAugment on the device (spec_augment, loader/spec_augment.py:68-115: time_warp :48-65 -> sparse_image_warp,
 * loader/sparse_image_warp.py:88-111, then frequency masks :98-104 and time masks :107-113; what `augmentation.spec_augment: True`
 * runs per clip, after normalisation and before _collate_fn).  With its single control point the reference's dense flow is zero
 * along frequency and affine along time: flow_t(f, t) = a_f f + a_t t + a_0; out[f][t] interpolates row f linearly at t - flow_t
 * with floor clamped to [0, T - 2] and the weight to [0, 1] (interpolate_bilinear, :357-408), T the clip's own frame count.
 *   warp_draw [N][12] f32 (device; null = no warp): i = randrange(W, T - W) (negative = no warp for the clip), d = randrange(-W, W),
 *     the nine values of randn(3, 3) / 1e10 (sparse_image_warp.py:170, row major), one pad.  Clips with T <= 2W frames are not
 *     warped (the reference raises ValueError there); W is time_warp's (default 5).
 *   fmask [N][MF][2], tmask [N][MT][2] int32 (device): start and width of every mask, width <= 0 = none; MF, MT <= 4; null iff 0.
 *   coef [N][3] f32 (device): (a_f, a_t, a_0); all zero = the clip is not warped.
 * ds2_spectrogram_aug = ds2_spectrogram with the augmentation folded into its write kernel (same ws; coef_out optional).
 * ds2_spec_augment_coef / ds2_spec_augment: the same two steps for a batch (N, 1, F, Tmax) f32 that exists already, any F, clip n
 * = the first frames[n] frames (device int32); out != in, frames >= frames[n] of out are zero. */
int ds2_spectrogram_aug(const float* wav, long ldw, const int* nsamples, int N, int Lmax, const float* basis, int reflect,
                        int normalize, float* out, void* ws, const float* warp_draw, int W, const int* fmask, int MF,
                        const int* tmask, int MT, float* coef_out, ds2_stream_t stream);
int ds2_spec_augment_coef(const float* x, int N, int F, int Tmax, const int* frames, const float* warp_draw, int W, float* coef,
                          ds2_stream_t stream);
int ds2_spec_augment(const float* in, float* out, int N, int F, int Tmax, const int* frames, const float* coef, const int* fmask,
                     int MF, const int* tmask, int MT, ds2_stream_t stream);

/* ---- running (causal) normalisation and the streaming front-end ----------------------------------------
 * normalize = 2.  With v[t][f] = log1p(|X[t][f]|) in fp32, s[t] = sum_f (double) v and q[t] = sum_f (double) v^2 (an order that
 * depends on f alone), the state (S, Q) is a STRICT left fold in frame order, S_t = S_(t-1) + s[t], Q_t = Q_(t-1) + q[t], and
 *   cnt_t = 161 (t + 1) + prior_cnt, mean_t = S_t / cnt_t, var_t = max((Q_t - cnt_t mean_t^2) / (cnt_t - 1), 0),
 *   rstd_t = 1 / max(sqrt(var_t), floor), out[f][t] = (v[t][f] - (float) mean_t) * (float) rstd_t          (all fp64 until the casts).
 * floor > 0 belongs to the mode: digital silence gives zeros, never NaN.  prior_frames > 0 starts the fold from pseudo-counts,
 * S0 = prior_mean 161 prior_frames, Q0 = (prior_std^2 + prior_mean^2) 161 prior_frames, prior_cnt = 161 prior_frames; 0 = none.
 * ds2_spectrogram_running: ds2_spectrogram (aug = 0; the arguments behind it are ignored) or ds2_spectrogram_aug (aug != 0) in this
 *   mode; the warp's two source frames and its control value are each normalised with their own frame's statistics.
 *   ws: ds2_spect_running_ws_bytes(N, Lmax).  N <= 65535.
 * The streaming form gives, for audio cut into feeds of ANY lengths, the frames of the one-shot call on the whole clip bit for bit
 * (zero centre padding only).  After G samples of a stream G / 160 frames are complete, frame t covers samples [160 t - 160,
 * 160 t + 160); the end of the utterance completes 1 + G / 160.  A slot keeps the samples that incomplete frames need (at most 319)
 * and (S, Q); the frame count is the caller's.
 * ds2_spect_stream_plan (host only): after samples_before samples, a feed of n_new more (final != 0: the utterance ends) -> out[0]
 *   frames complete before, out[1] frames emitted, out[2] window samples in front of the new ones (160 + samples_before % 160, the
 *   left padding included), out[3] the window's length (with the 160 zeros behind a final feed), out[4] the samples carried on (0
 *   after a final feed), out[5] the clip position of the window's first sample (-160 inside the left padding).
 * ds2_spect_stream_state_bytes(S): [S][2] f64 + [S][320] f32; ds2_spect_stream_ws_bytes(n_rows, max_new, Tc): the workspace.
 * ds2_spect_stream_feed: row r reads its n_new <= max_new <= ldw new samples from wav[src] and writes out[r] of out (n_rows, 1, 161,
 *   Tc) f32, frames >= emit zero; Tc >= every emit, Tc = 0 moves the carries alone.  A row with fresh != 0 reads its slot's carry as
 *   the 160 zeros of the left padding and its statistics as the prior, whatever the slot holds (carried must be 0 then).
 *   normalize 0 (raw log-magnitudes, no statistics) or 2; 1 is refused: per-utterance statistics are not causal.  The table lives
 *   on the device, so the entry cannot check it: slots distinct and in [0, S), src inside wav, the counts those of the plan.
 * DS2_ERR_ARG: a null buffer that is read or written, N or n_rows outside [1, 65535], S < n_rows, floor <= 0, a negative or NaN
 *   prior, Tc beyond what max_new samples can complete. */
typedef struct ds2_spect_stream_row {
  int32_t slot;          /* the stream's state slot, 0 <= slot < S */
  int32_t src;           /* the stream's row of wav */
  int32_t carried;       /* samples the window takes from the slot's carry (0 for a fresh slot) */
  int32_t n_new;         /* new samples */
  int32_t frames_before; /* frames of the stream emitted before this feed */
  int32_t emit;          /* frames this feed emits */
  int32_t final;         /* the utterance ends with this feed */
  int32_t fresh;         /* the slot's carry and statistics read as those of a new stream */
} ds2_spect_stream_row;
long ds2_spect_running_ws_bytes(int N, int Lmax);
int ds2_spectrogram_running(const float* wav, long ldw, const int* nsamples, int N, int Lmax, const float* basis, int reflect,
                            double floor, double prior_mean, double prior_std, double prior_frames, float* out, void* ws, int aug,
                            const float* warp_draw, int W, const int* fmask, int MF, const int* tmask, int MT, float* coef_out,
                            ds2_stream_t stream);
int ds2_spect_stream_plan(long samples_before, int n_new, int final, int* out);
long ds2_spect_stream_state_bytes(int S);
long ds2_spect_stream_ws_bytes(int n_rows, int max_new, int Tc);
int ds2_spect_stream_feed(const float* wav, long ldw, const ds2_spect_stream_row* rows, int n_rows, int max_new, int Tc, int S,
                          const float* basis, int normalize, double floor, double prior_mean, double prior_std, double prior_frames,
                          void* state, float* out, void* ws, ds2_stream_t stream);

/* ---- waveform augmentation on the device (what SpectrogramParser.parse_audio does to the samples before the STFT,
 * loader/data_loader.py:151-159: load_randomly_augmented_audio, :377-404 = sox `tempo t gain g`, then NoiseInjection.inject_noise,
 * :97-128).  Every entry works on a batch wav [N][ldw] f32 (clip n = the first nsamples[n] entries of row n; nsamples [N] int32 on
 * the device), writes out of place into out [N][ldo] and writes the entries of a row beyond the clip's own samples as zero.  The
 * random draws are the caller's (augment.WaveAugment.draw).
 * Tempo = the project's own WSOLA with sox's default `tempo` parameters at 16 kHz: segment 1312, 234 candidate offsets, overlap 192;
 * ADV = 1120.  start(k) = floor(k * tempo * 1120) in fp64; S = the number of k with start(k) + 192 <= nsamples;
 * out_len = (S - 1) * 1120 + min(1312, nsamples - start(S - 1)).  Segment 0 sits at p(0) = 0; segment k >= 1 at p(k) = start(k) + d,
 * d in [0, 234) the lowest arg-max of the fp32 dot product of x[p(k-1) + 1120 + j] with x[start(k) + d + j], j in [0, 192); reads at or
 * beyond nsamples are zero.  out[1120 k + j] = x[p(k) + j], cross-faded over j < 192 as a + (j / 192) (x[p(k) + j] - a) with
 * a = x[p(k-1) + 1120 + j]; the last segment runs to out_len.  A clip with nsamples < 1546 or a tempo outside [0.1, 10] is copied.
 *   tempo [N] f32 (device; null = every clip is copied; exactly 1.0f still runs the algorithm)
 *   nsamples_out [N] int32 (device): min(out_len, ldo), the sample counts of out
 *   offsets [N][Smax] int32 (device; may be null with Smax 0): the chosen d of every segment (0 for segment 0), -1 beyond S
 * ds2_wsola_segments / ds2_wsola_out_len: S (0 = copied) and out_len of one clip, host-only queries.  DS2_ERR_ARG: a null wav,
 * nsamples, out or nsamples_out, wav == out, N, ldw or ldo < 1, ldo >= 2^31, Smax < 0.
 * Gain and noise: y = clamp(gain[n] * x, -1, 1) (gain [N] f32 LINEAR factors, 10^(dB / 20); null = x unchanged, not clamped), then
 * out = y + scale * noise[noise_off[n] + noise_start[n] + i] with scale = level[n] * sqrt(sum y^2 / sum noise^2), both sums over the
 * clip's own samples (data_loader.py:125-127, rms(data) / rms(noise)).  bank: bank_len f32 noise samples (recordings back to back),
 * noise_off [N] int64 the recording's first sample (negative = no noise for the clip), noise_start [N] int32 the crop's first sample
 * inside it, level [N] f32 (<= 0 = no noise for the clip; a null level = no noise at all, bank / noise_off / noise_start unused).
 * Reads outside the bank are zero; a crop without energy adds nothing.
 * ds2_wave_energy writes the sums as fixed-order fp64 partials [N][8][2] (data, noise; block b of a clip sums the samples
 * i with (i / 256) % 8 == b) into ws, ds2_wave_ws_bytes(N) bytes, 8-byte aligned; ds2_wave_mix reads them (ws may be null when level
 * is).  DS2_ERR_ARG: a null wav, nsamples or out, wav == out, N < 1 or > 65535, a level without bank, offsets, starts or ws. */
int ds2_wsola_segments(int nsamples, float tempo);
long ds2_wsola_out_len(int nsamples, float tempo);
int ds2_wsola(const float* wav, long ldw, const int* nsamples, const float* tempo, int N, float* out, long ldo, int* nsamples_out,
              int* offsets, int Smax, ds2_stream_t stream);
long ds2_wave_ws_bytes(int N);
int ds2_wave_energy(const float* wav, long ldw, const int* nsamples, int N, const float* gain, const float* level,
                    const float* bank, long bank_len, const long long* noise_off, const int* noise_start, void* ws,
                    ds2_stream_t stream);
int ds2_wave_mix(const float* wav, long ldw, const int* nsamples, int N, const float* gain, const float* level, const float* bank,
                 long bank_len, const long long* noise_off, const int* noise_start, const void* ws, float* out, long ldo,
                 ds2_stream_t stream);

/* ---- reverberation (DESIGN.md section 7.1 "Reverberation"; the reference has none, the rule is the project's own): every clip
 * convolved with its room impulse response, time-aligned on the response's direct-path tap.  For clip n with L = nsamples[n] samples
 * x, a response h of K = rir_len[n] taps at bank[rir_off[n] ..] and its peak index p = rir_peak[n] (0 <= p < K):
 *   out[i] = sum_{k = 0}^{K - 1} h[k] * x[i + p - k]   for 0 <= i < L,   x = 0 outside [0, L)
 *   out[i] = 0                                         for L <= i < ldo
 * so the output has the input's length and its timing (frame counts, transcripts, alignments and the noise step's data length do
 * not change); the reverberant tail beyond the clip's end is cut.  All arithmetic is fp32 with fp32 accumulation, nothing is
 * clamped.  Summation order of output i: acc = +0, then acc = fma(h[k], x[i + p - k], acc) over the blocks q = 0, 1, .. (K + 30) / 32
 * of 32 taps in rising q, inside a block k = 32 q + (i mod 32) - r in rising r = 0 .. 31 (k falls); a k outside [0, K) enters
 * as h = 0.  The order depends on i mod 32 and K alone -- never on the row, N, ldw / ldo or the other rows --, no atomics, no sum
 * is split: a clip's output bits are the same wherever it sits.  (Adding to +0 turns a -0 sample into +0.)
 *   bank: bank_len f32 on the device, the responses back to back; reads outside the bank are zero
 *   rir_off [N] int64, rir_len / rir_peak [N] int32 (device).  rir_off[n] < 0: the clip is copied bit for bit (zeros beyond L);
 *   a null rir_off copies every clip (bank / rir_len / rir_peak unused).  rir_len[n] < 1 gives zeros.
 * The kernel is the direct-form FIR as a block-Toeplitz product on v_mfma_f32_32x32x2_f32; a row costs its own K, a copied row
 * nothing.  ds2_reverb_tile(): the consecutive outputs one workgroup computes (host-only query).
 * DS2_ERR_ARG: a null wav, nsamples or out, wav == out, N < 1 or > 65535, ldw or ldo < 1, a rir_off without bank, rir_len or
 * rir_peak; nothing is launched then. */
int ds2_reverb_tile(void);
int ds2_reverb(const float* wav, long ldw, const int* nsamples, int N, const float* bank, long bank_len, const long long* rir_off,
               const int* rir_len, const int* rir_peak, float* out, long ldo, ds2_stream_t stream);

/* ---- rational polyphase resampling to 16 kHz (the reference converts its corpora with sox `rate` offline).
 * g = gcd(in_rate, 16000), U = 16000 / g, D = in_rate / g, W = the half-width in input samples, taps [U][2W] f32 on the device,
 * 8-byte aligned, U * 2W * 4 <= 128 KiB (resample.Resampler builds them on the host in fp64).  Output m of a clip x of n samples:
 *   n0 = floor(m D / U), p = (m D) mod U (64-bit), y[m] = sum_j taps[p][j] x[n0 - W + 1 + j], x = 0 outside [0, n);  m < ceil(n U / D).
 * The sum is acc = fma(taps[p][j], x, acc) from acc = 0 in rising j, in every entry: the order depends on the tap index alone.
 * ds2_resample_out_len(n, U, D) = ceil(n U / D), ds2_resample_tile(U, D, W) = the consecutive outputs one workgroup computes: host
 *   only.  ds2_resample: wav [N][ldw], nsamples [N] int32 (device) -> out [N][ldo], zero beyond a clip's outputs, and nsamples_out
 *   [N] int32 (device) = min(out_len, ldo).
 * Streaming: after G samples of a stream that has not ended, E(G) = 0 for G <= W, else ceil((G - W) U / D) outputs exist (those
 *   whose last tap n0 + W has arrived); the end of the utterance completes ceil(G U / D).  A slot keeps the input samples from
 *   max(0, n0(E) - W + 1) on, at most 2W - 1.
 * ds2_resample_plan (host only): after samples_before samples, a feed of n_new more (final != 0: the utterance ends) -> out[0]
 *   outputs before, out[1] outputs emitted, out[2] samples taken from the carry, out[3] samples carried on (0 after a final
 *   feed), out[4] the clip position of the first carried sample.
 * ds2_resample_stream_state_bytes(S, W): [S][2W] f32; ds2_resample_stream_ws_bytes(n_rows, W): [n_rows][2W] f32.
 * ds2_resample_stream_feed: row r reads its n_new <= max_new <= ldw new samples from wav[src] and writes its emit <= max_emit <=
 *   ldo outputs to out[r] (out [n_rows][ldo]), zeros from emit to max_emit; max_emit = 0 moves the carries alone.  A row with
 *   fresh != 0 reads its slot's carry as empty, whatever the slot holds (carried and out_before must be 0 then); a final row
 *   leaves its slot as it is.  The table lives on the device (8-byte aligned), so the entry cannot check it: slots distinct
 *   (a slot outside [0, S) is skipped), src inside wav, the counts those of the plan.
 * DS2_ERR_ARG: a null buffer that is read or written, wav == out, N or n_rows outside [1, 65535], S < n_rows, U, D or W < 1, a
 *   table over 128 KiB, ldw < max_new, ldo < max_emit; DS2_ERR_ALIGN: taps or rows not 8-byte aligned.  Nothing is launched then. */
typedef struct ds2_resample_stream_row {
  int32_t slot;          /* the stream's state slot, 0 <= slot < S */
  int32_t src;           /* the stream's row of wav */
  int32_t carried;       /* samples taken from the slot's carry (0 for a fresh slot) */
  int32_t n_new;         /* new samples */
  int64_t out_before;    /* outputs of the stream that exist before this feed */
  int32_t emit;          /* outputs this feed emits */
  int32_t final;         /* the utterance ends with this feed */
  int32_t fresh;         /* the slot's carry reads as that of a new stream */
  int32_t pad;           /* ds2_resample_stream_feed_mixed: the row's class; ds2_resample_stream_feed does not read it */
} ds2_resample_stream_row;
long ds2_resample_out_len(long n, int U, int D);
int ds2_resample_tile(int U, int D, int W);
int ds2_resample_plan(long samples_before, int n_new, int final, int U, int D, int W, long* out);
int ds2_resample(const float* wav, long ldw, const int* nsamples, int N, const float* taps, int U, int D, int W, float* out, long ldo,
                 int* nsamples_out, ds2_stream_t stream);
long ds2_resample_stream_state_bytes(int S, int W);
long ds2_resample_stream_ws_bytes(int n_rows, int W);
int ds2_resample_stream_feed(const float* wav, long ldw, const ds2_resample_stream_row* rows, int n_rows, int max_new, int max_emit, int S,
                             const float* taps, int U, int D, int W, void* state, float* out, long ldo, void* ws, ds2_stream_t stream);

/* Mixed rates: U, D, W and the table belong to the row, not to the launch.  A CLASS is one (U, D, W, taps), what the entries above
 * take; a call carries C <= 16 of them.  (1, 1, 0) is the COPY class, y[m] = x[m] bit for bit (16 kHz rows ride in the same
 * launch); it has no table.  A row of a mixed call is, bit for bit, the row of the single-rate call with its class's numbers, and
 * a streamed row the one-shot row however it is cut into feeds.
 * ds2_resample_classes (host only): udw [C][3] = (U, D, W) per class -> table [C], with each class's tile shape (the one
 *   ds2_resample_tile reports) and taps_off, and *taps_floats = the floats of the taps buffer: the tables one behind the other in
 *   class order, class c's taps_off floats in (always even: 8-byte aligned).  The caller keeps the table and uploads the same bytes
 *   as the device table; the entries take both, the host's for the launch shape, the device's for the kernels.
 * ds2_resample_mixed: ds2_resample with cls [N] int32 (device), the class of each row.  nsamples_out = min(out_len of the row's
 *   class, ldo).  A row whose class is outside [0, C) computes nothing: zeros and a count of 0.
 * ds2_resample_stream_feed_mixed: ds2_resample_stream_feed with the class in the row's pad word.  state [S][2 Wmax] f32 and ws
 *   [n_rows][2 Wmax] f32 (the _mixed size queries), Wmax >= every W of the table and >= 1; a slot keeps at most 2 W - 1 samples
 *   of its class.  A fresh row reads its slot's carry as empty, whatever a stream of another class left there.  A row whose
 *   class is outside [0, C) writes zeros and leaves its slot alone; the copy class emits its n_new samples and carries nothing.
 * One compute launch per call whatever C is (streaming adds the carry launch).
 * DS2_ERR_ARG: as above, and C outside [1, 16], a class that is neither the copy class nor has U, D, W >= 1 and a table of at most
 *   128 KiB, a host table whose tile shape is not the one ds2_resample_classes gives, Wmax < a W, taps null with a class that has
 *   a table; DS2_ERR_ALIGN: taps, rows or classes_dev not 8-byte aligned, an odd taps_off.  Nothing is launched then. */
typedef struct ds2_resample_class {
  int32_t U, D, W;
  int32_t nt, P, K;      /* threads that work, outputs between two outputs of a thread, outputs per thread */
  int32_t tile;          /* P K: the consecutive outputs one workgroup computes */
  int32_t cap;           /* floats of the input span staged in LDS, 0 = read from global memory */
  int64_t taps_off;      /* floats in front of the class's table in the taps buffer */
} ds2_resample_class;
int ds2_resample_classes(const int* udw, int C, ds2_resample_class* table, long* taps_floats);
int ds2_resample_mixed(const float* wav, long ldw, const int* nsamples, const int* cls, int N, const ds2_resample_class* classes,
                       const ds2_resample_class* classes_dev, int C, const float* taps, float* out, long ldo, int* nsamples_out,
                       ds2_stream_t stream);
long ds2_resample_stream_state_bytes_mixed(int S, int Wmax);
long ds2_resample_stream_ws_bytes_mixed(int n_rows, int Wmax);
int ds2_resample_stream_feed_mixed(const float* wav, long ldw, const ds2_resample_stream_row* rows, int n_rows, int max_new, int max_emit,
                                   int S, const ds2_resample_class* classes, const ds2_resample_class* classes_dev, int C, const float* taps,
                                   int Wmax, void* state, float* out, long ldo, void* ws, ds2_stream_t stream);

/* ---- greedy CTC decoding on the device (validation_step, model.py:256 -> GreedyDecoder.decode, decoder.py:164-181) -------
 * x[n*stride_n + t*stride_t + c] f32 scores (probabilities or logits), C <= 64; sizes [N] int32 on the device (null = T).
 * Per sample: arg-max per frame (first maximum), repeats collapsed, blanks dropped.  tokens / offsets [N][T] int32 (the first
 * counts[n] entries of row n are valid: label index and its frame), counts [N]. */
int ds2_greedy_decode(const float* x, long stride_n, long stride_t, int N, int T, int C, const int* sizes, int blank,
                      int* tokens, int* offsets, int* counts, ds2_stream_t stream);

/* ds2_greedy_decode on one chunk (N, Tc, C) of N streams.  carry: [N][2] int32 on the device, per stream (arg-max of its last
 * frame, frames consumed); all zero for a fresh stream, updated by the call.  sizes[n] == 0 leaves stream n as it is.
 * tokens / offsets [N][Tc]: the counts[n] labels that this chunk adds to stream n and their frames counted from the start of the
 * stream.  Greedy output is append-only: the chunks' outputs, concatenated, are ds2_greedy_decode's on the concatenated input.
 * Tc >= 1: there is no output stage to run on its own, so unlike ds2_beam_stream_feed an empty chunk is DS2_ERR_ARG (the
 * wrappers return before the call).  The consumed-frame counter is an int32 that nothing bounds: a stream must be reset before
 * it has taken 2^31 - 1 frames. */
int ds2_greedy_stream_feed(const float* x, long stride_n, long stride_t, int N, int Tc, int C, const int* sizes, int blank,
                           int* carry, int* tokens, int* offsets, int* counts, ds2_stream_t stream);

/* ---- CTC prefix beam search on the device (BeamCTCDecoder, reference decoder.py:56-117) ---------------
 * x[n*stride_n + t*stride_t + c] f32 probabilities, C <= 8192; sizes [N] int32 on the device (null = T); 1 <= B <= 256,
 * cutoff_top_n >= 1 with min(cutoff_top_n, C) <= 64; cutoff_prob < 1 also cuts each frame at that cumulative probability.
 * Outputs (device): tokens / offsets [N][B][T] int32 (the first lens[n][b] entries of row (n, b): label index and its frame),
 * lens [N][B] int32, scores [N][B] f32 = -log p of the prefix (ctcdecode's convention; +inf for a rank without a beam).
 * ws: ds2_beam_ws_bytes(N, T, B) bytes of device memory, 256-byte aligned (host-only size query). */
long ds2_beam_ws_bytes(int N, int T, int B);
int ds2_beam_decode(const float* x, long stride_n, long stride_t, int N, int T, int C, const int* sizes, int blank, int B,
                    int cutoff_top_n, float cutoff_prob, int* tokens, int* offsets, int* lens, float* scores, void* ws,
                    ds2_stream_t stream);

/* The same search with a word n-gram language model (DESIGN.md "ds2_beam", language model; tables built by lm.py).
 * space: the label that ends a word (!= blank).  word_table / ngram_table: open-addressing tables [slots][2] of 64-bit words
 * (key, value) in device memory, 16-byte aligned, slots a power of two in [2, 2^31]; a free slot holds ~0.
 *   word table: key = hash of a word prefix's label string (the beam strings' recurrence), value = word id, -1 for a proper prefix
 *   n-gram table: key = hash of the id tuple, value = fp32 bits of log10 p | fp32 bits of log10 backoff << 32
 * order in [1, 5]; bos = id of <s>.  A word event adds alpha * ln P(word | context) + beta to the beam's lm; lexicon != 0 drops
 * candidates whose partial word is no prefix of a vocabulary word.  scores [N][B] = -(log p + lm), the quantity that ranks the
 * beams; acoustic [N][B] (may be null) = -log p of the same ranks.  Everything else, ws included, as for ds2_beam_decode.
 * DS2_ERR_ARG: order or space out of range, space == blank, a null table, slots not a power of two. */
int ds2_beam_decode_lm(const float* x, long stride_n, long stride_t, int N, int T, int C, const int* sizes, int blank, int B,
                       int cutoff_top_n, float cutoff_prob, int space, const void* word_table, long word_slots,
                       const void* ngram_table, long ngram_slots, int order, int bos, float alpha, float beta, int lexicon,
                       int* tokens, int* offsets, int* lens, float* scores, float* acoustic, void* ws, ds2_stream_t stream);

/* ds2_beam_decode_lm for a grid of G weight points (alphas[g], betas[g]), both device f32 [G], 1 <= G <= 65535: the frames are
 * pruned once and G x N workgroups search, each in a node pool of its own.  Of every (point, sample) only the top beam after the
 * end-of-utterance re-rank is written: tokens / offsets [G][N][T] int32 (offsets may be null), lens / scores / acoustic [G][N]
 * (acoustic may be null).  Row (g, n) equals rank 0 of sample n of ds2_beam_decode_lm(alpha = alphas[g], beta = betas[g]), bit for
 * bit.  ws: ds2_beam_grid_ws_bytes(G, N, T, B) bytes, 256-byte aligned; ds2_beam_grid_ws_bytes(1, ..) == ds2_beam_ws_bytes(..) and
 * every further point adds the node pools only (affine in G).  DS2_ERR_ARG: G out of range, null alphas or betas, and all of
 * ds2_beam_decode_lm's. */
long ds2_beam_grid_ws_bytes(int G, int N, int T, int B);
int ds2_beam_decode_lm_grid(const float* x, long stride_n, long stride_t, int N, int T, int C, const int* sizes, int blank, int B,
                            int cutoff_top_n, float cutoff_prob, int space, const void* word_table, long word_slots,
                            const void* ngram_table, long ngram_slots, int order, int bos, int lexicon, int G, const float* alphas,
                            const float* betas, int* tokens, int* offsets, int* lens, float* scores, float* acoustic, void* ws,
                            ds2_stream_t stream);

/* ---- character language model (DESIGN.md "ds2_beam", character language model) ---------------------------------------------
 * The search with an n-gram model whose units are the labels themselves (label sets without word boundaries): every new label is
 * an event of the model, lm += alpha * ln P(label | the last order - 1 labels) + beta, with <s> in front of a short string.
 * After the shared leading arguments comes one block: cid [C] device int32, the unigram id of every class, -1 where the file
 * has none (the blank's entry is not read); ngram_table / ngram_slots as for ds2_beam_decode_lm; order in [1, 5]; bos = id of
 * <s>; alpha, beta (the grid form: G, alphas, betas as ds2_beam_decode_lm_grid).  There is no word table, no lexicon, no
 * end-of-utterance term and no re-rank: scores = -(log p + lm) of the last selection's ranks, acoustic (may be null) = -log p.
 * With alpha = beta = 0 the outputs are ds2_beam_decode's bit for bit.  The stream form works on a buffer sized with flags = 5
 * (bit 2 = "the language model scores characters", valid only with bit 0 and without bit 1); its state has the word LM's size.
 * Outputs, ws, bounds and error codes as for the _lm counterparts; DS2_ERR_ARG also for a null cid. */
int ds2_beam_decode_clm(const float* x, long stride_n, long stride_t, int N, int T, int C, const int* sizes, int blank, int B,
                        int cutoff_top_n, float cutoff_prob, const int* cid, const void* ngram_table, long ngram_slots, int order,
                        int bos, float alpha, float beta, int* tokens, int* offsets, int* lens, float* scores, float* acoustic,
                        void* ws, ds2_stream_t stream);
int ds2_beam_decode_clm_grid(const float* x, long stride_n, long stride_t, int N, int T, int C, const int* sizes, int blank, int B,
                             int cutoff_top_n, float cutoff_prob, const int* cid, const void* ngram_table, long ngram_slots,
                             int order, int bos, int G, const float* alphas, const float* betas, int* tokens, int* offsets,
                             int* lens, float* scores, float* acoustic, void* ws, ds2_stream_t stream);
int ds2_beam_stream_feed_clm(const float* x, long stride_n, long stride_t, int N, int Tc, int C, const int* sizes, int blank, int B,
                             int cutoff_top_n, float cutoff_prob, const int* cid, const void* ngram_table, long ngram_slots,
                             int order, int bos, float alpha, float beta, void* state, int max_frames, int* tokens, int* offsets,
                             long row_stride, int out_ranks, int* lens, float* scores, float* acoustic, void* ws,
                             ds2_stream_t stream);

/* ---- hot words (DESIGN.md "ds2_beam", hot words) ---------------------------------------------------------------------------
 * ds2_beam_decode / ds2_beam_decode_lm with a table of hot phrases: a beam earns a boost while its string ends in a prefix of a
 * phrase, and keeps the boost of every phrase it has completed.  hot_table: the open-addressing table of hotwords.build_table,
 * [hot_slots][2] 64-bit words (key = 61-bit string hash of a phrase prefix, value = v bits | c bits << 32 | whole phrase << 63),
 * hot_slots a power of two >= 2, 16-byte aligned.  space: the label that ends a word (not the blank).  scores = -(log p + hot_end),
 * with an LM -((log p + lm) + hot_end): the total that ranks the beams; acoustic [N][B] (may be null) = -log p of the same ranks.
 * hot_oov_logp (finite): ln P charged to a word event whose word is out of vocabulary but covered by a hot phrase.  Everything
 * else as ds2_beam_decode / ds2_beam_decode_lm, whose results these calls give bit for bit when every weight in the table is 0
 * (with an LM: and every phrase word is in the vocabulary).  DS2_ERR_ARG: a null table, hot_slots no power of two >= 2, space
 * out of range or the blank, a hot_oov_logp that is not finite, and all of the siblings'. */
int ds2_beam_decode_hot(const float* x, long stride_n, long stride_t, int N, int T, int C, const int* sizes, int blank, int B,
                        int cutoff_top_n, float cutoff_prob, int space, const void* hot_table, long hot_slots, int* tokens,
                        int* offsets, int* lens, float* scores, float* acoustic, void* ws, ds2_stream_t stream);
int ds2_beam_decode_lm_hot(const float* x, long stride_n, long stride_t, int N, int T, int C, const int* sizes, int blank, int B,
                           int cutoff_top_n, float cutoff_prob, int space, const void* word_table, long word_slots,
                           const void* ngram_table, long ngram_slots, int order, int bos, float alpha, float beta, int lexicon,
                           const void* hot_table, long hot_slots, float hot_oov_logp, int* tokens, int* offsets, int* lens,
                           float* scores, float* acoustic, void* ws, ds2_stream_t stream);

/* ---- resumable CTC prefix beam search: N streams fed chunk by chunk (DESIGN.md "ds2_beam_stream") --------------------------
 * After feeds that delivered frames [0, t_n) of stream n, the output stage gives what ds2_beam_decode / ds2_beam_decode_lm give on
 * those t_n frames, bit for bit (labels, frames, lengths, scores, acoustic scores).
 * state: one device buffer per session of ds2_beam_stream_bytes(N, B, max_frames, lm) bytes, 256-byte aligned (host-only size
 *   query; 0 for N, B or max_frames <= 0; lm != 0 adds the language-model fields).  It holds per stream a header of four int32
 *   (frames consumed, live beams, overflow flag, unused) and the beams' fields as arrays of B entries, at a 256-byte aligned
 *   stride of 16 + 32 * B (+ 36 * B with an LM) bytes, which ds2_beam_stream_state_stride(B, lm) returns (host-only; 0 for
 *   B <= 0), then the node pool [N][max_frames + 1][B] x (parent, label, frame) int32:
 *   12 * B bytes per frame and stream.  N, B, max_frames, lm, blank, the cutoffs and the LM arguments are the session's: the same
 *   in every call on one buffer.
 * ds2_beam_stream_reset: the streams with mask[n] != 0 (mask [N] int32 on the device, null = all) start again from the empty
 *   beam; the others are untouched.  A new buffer is reset as a whole before its first feed.
 * ds2_beam_stream_feed: x is the chunk (N, Tc, C) with ds2_beam_decode's strides and limits; sizes [N] int32 on the device
 *   (null = Tc) says how many of its frames each stream takes, 0 leaving the stream as it is.  A stream whose consumed count would
 *   pass max_frames takes nothing and has its overflow flag set (until it is reset); the pool is never written beyond.
 *   tokens / offsets / lens / scores are all null (no output stage) or all given: then the best out_ranks beams of every stream
 *   are written, 1 <= out_ranks <= B: rows (n, b), b < out_ranks, of tokens / offsets lie row_stride ints apart, row_stride >=
 *   the largest consumed count (labels past a shorter row are not written); lens / scores [N][out_ranks].  The output stage
 *   reads the state and leaves it unchanged.  Tc == 0 runs the output stage alone (x, sizes, ws unused).
 *   ws: ds2_beam_stream_ws_bytes(N, Tc) bytes (the chunk's kept lists), 256-byte aligned; needed during the call only.
 * ds2_beam_stream_feed_lm: the same with the language model of ds2_beam_decode_lm; the output stage includes the end-of-utterance
 *   bonus and re-rank, which always look at all the live beams; acoustic [N][out_ranks] may be null.
 *   The consumed count never passes max_frames, so it needs no bound of its own.
 * flags (the former `lm` argument of the two size queries and of ds2_beam_stream_reset; 0 and 1 mean what they meant): bit 0 a
 *   language model, bit 1 hot words, bit 2 (only as flags = 5) a character language model, whose fields take the word LM's
 *   36 * B bytes; any other word gives size 0 / DS2_ERR_ARG.  Hot words add, from the next multiple of 8 bytes
 *   after the other fields, 24 * B bytes (match hash, done, v, space value, flags), and 8 * B more (the partial-word hash) when
 *   there is no LM: a stride of 16 + 64 * B bytes without an LM and 16 + align8(68 * B) + 24 * B with one, rounded up to 256.
 * ds2_beam_stream_feed_hot / _feed_lm_hot: the same with the hot words of ds2_beam_decode_hot / _lm_hot, on a buffer sized with
 *   flags 2 / 3; the output stage includes hot_end and the re-rank.
 * DS2_ERR_ARG: as ds2_beam_decode(_lm); outputs given in part, or out_ranks outside [1, B] with them; Tc == 0 without outputs; (max_frames + 1) * B > 2^31 - 1. */
long ds2_beam_stream_bytes(int N, int B, int max_frames, int flags);
long ds2_beam_stream_ws_bytes(int N, int Tc);
long ds2_beam_stream_state_stride(int B, int flags);
int ds2_beam_stream_reset(void* state, int N, int B, int max_frames, int flags, const int* mask, ds2_stream_t stream);
int ds2_beam_stream_feed(const float* x, long stride_n, long stride_t, int N, int Tc, int C, const int* sizes, int blank, int B,
                         int cutoff_top_n, float cutoff_prob, void* state, int max_frames, int* tokens, int* offsets,
                         long row_stride, int out_ranks, int* lens, float* scores, void* ws, ds2_stream_t stream);
int ds2_beam_stream_feed_lm(const float* x, long stride_n, long stride_t, int N, int Tc, int C, const int* sizes, int blank, int B,
                            int cutoff_top_n, float cutoff_prob, int space, const void* word_table, long word_slots,
                            const void* ngram_table, long ngram_slots, int order, int bos, float alpha, float beta, int lexicon,
                            void* state, int max_frames, int* tokens, int* offsets, long row_stride, int out_ranks, int* lens,
                            float* scores, float* acoustic, void* ws, ds2_stream_t stream);
int ds2_beam_stream_feed_hot(const float* x, long stride_n, long stride_t, int N, int Tc, int C, const int* sizes, int blank, int B,
                             int cutoff_top_n, float cutoff_prob, int space, const void* hot_table, long hot_slots, void* state,
                             int max_frames, int* tokens, int* offsets, long row_stride, int out_ranks, int* lens, float* scores,
                             float* acoustic, void* ws, ds2_stream_t stream);
int ds2_beam_stream_feed_lm_hot(const float* x, long stride_n, long stride_t, int N, int Tc, int C, const int* sizes, int blank,
                                int B, int cutoff_top_n, float cutoff_prob, int space, const void* word_table, long word_slots,
                                const void* ngram_table, long ngram_slots, int order, int bos, float alpha, float beta, int lexicon,
                                const void* hot_table, long hot_slots, float hot_oov_logp, void* state, int max_frames, int* tokens,
                                int* offsets, long row_stride, int out_ranks, int* lens, float* scores, float* acoustic, void* ws,
                                ds2_stream_t stream);

/* ---- endpointing: endless streams cut into utterances on the device ------------------------------
 * Frame t of a stream is silent iff x[t][blank] > blank_threshold (fp32, strict; a NaN is not silent).  A segment starts at frame
 * s (0, or one past the previous endpoint) and ends at the first t where, in this order, 1 "silence": a non-silent frame in
 * [s, t] and at least min_trailing silent frames ending at t; 2 "leading": no non-silent frame and at least max_leading silent
 * ones; 3 "length": t - s + 1 == max_segment.  Reason 4 "final" is ds2_endpoint_close's.
 * state: ds2_endpoint_state_bytes(N) bytes, 16-byte aligned: per stream eight int32 (segment start as an absolute frame,
 *   trailing, spoken, frames consumed, segments finished, three reserved).  The counters are int32: 2^31 frames per stream.
 * ds2_endpoint_reset: the streams with mask[n] != 0 (mask [N] int32 on the device, null = all) start again at frame 0, segment 0.
 * ds2_endpoint_feed: x is the chunk (N, Tc, C) with ds2_beam_stream_feed's strides; sizes [N] int32 on the device (null = Tc).
 *   Frames at and beyond sizes[n] are never read; sizes[n] == 0 leaves the state of stream n bitwise as it is.  The state
 *   advances to the first endpoint and stops: cut[n] = the frames of the chunk that belong to the open segment (sizes[n] without
 *   an endpoint), rest[n] = sizes[n] - cut[n]; events [4][N] int32 = rows (reason, start, end, index), all 0 without an endpoint,
 *   so the first row is a mask for ds2_beam_stream_reset.  One wave per stream, 64 frames per step.
 * ds2_endpoint_close: the open segment of the masked streams ends with reason 4 at the last frame consumed (end = start - 1 for
 *   an empty one); events as above.
 * ds2_endpoint_gather: y (N, Tc, C) contiguous, y[n][i] = x[n][cut[n] + i] for i < rest[n]: the frames after the endpoint at the
 *   front of a second chunk, for a second feed with sizes = rest.  Nothing else of y is written, nothing beyond cut + rest read.
 * ds2_endpoint_commit: for the streams with a non-zero reason, the event and the rows that a beam feed's output stage wrote
 *   (its tokens / offsets / row_stride / out_ranks / lens / scores / acoustic arguments; acoustic null = scores) are copied to
 *   slot pending[n] of the stream's ring and pending[n] grows by one; a stream whose `slots` slots are full is skipped.  ring:
 *   ds2_endpoint_ring_bytes(N, slots, ranks, row_stride) bytes of [N][slots] slots, each 4 + 3 * ranks + 2 * ranks * row_stride
 *   int32 words: event, lens, scores, acoustic, tokens, offsets.  pending [N] int32 on the device; the caller zeroes it when it
 *   has fetched the ring.
 * DS2_ERR_ARG: a null pointer other than sizes / mask / acoustic, N, C, slots, ranks or row_stride < 1, Tc < 1, a blank outside
 *   [0, C), a threshold outside (0, 1), a count < 1.  DS2_ERR_ALIGN: a state that is not 16-byte aligned.  Size queries: 0. */
long ds2_endpoint_state_bytes(int N);
long ds2_endpoint_ring_bytes(int N, int slots, int ranks, long row_stride);
int ds2_endpoint_reset(void* state, int N, const int* mask, ds2_stream_t stream);
int ds2_endpoint_feed(const float* x, long stride_n, long stride_t, int N, int Tc, int C, const int* sizes, int blank,
                      float blank_threshold, int min_trailing, int max_leading, int max_segment, void* state, int* cut, int* rest,
                      int* events, ds2_stream_t stream);
int ds2_endpoint_close(void* state, int N, const int* mask, int* events, ds2_stream_t stream);
int ds2_endpoint_gather(const float* x, long stride_n, long stride_t, int N, int Tc, int C, const int* cut, const int* rest, float* y,
                        ds2_stream_t stream);
int ds2_endpoint_commit(const int* events, const int* tokens, const int* offsets, long row_stride, int ranks, const int* lens,
                        const float* scores, const float* acoustic, int N, void* ring, int* pending, int slots, ds2_stream_t stream);

/* ---- keyword spotting on the CTC outputs, one-shot and streamed ------------------------------------
 * THE RULE (tests/kws_reference.py restates it in numpy; every word is pinned by tests).
 * Frame scores: for frame t with class scores x_t[c], r_t[c] = lp_t[c] - max_c' lp_t[c'] <= 0, where lp = x for mode 0 (logits)
 *   and 2 (log-probabilities) and lp = logf(x) for mode 1 (probabilities); the log-normaliser cancels, so logits need no
 *   log-sum-exp.  A detection's score is a log-likelihood ratio: the best path through the keyword on its frames against the
 *   greedy path on the same frames; it is 0 exactly when the greedy path spells the keyword there.
 * Lattice: a keyword is labels y_1..y_L, 1 <= L <= 64, never the blank; the space label may stand anywhere.  2L - 1 states
 *   y_1, blank, y_2, blank, ..., y_L (no leading or trailing blank), each with a value v (fp32) and the absolute frame b at which
 *   its path started.  At frame t state 0 takes max(v_{t-1}(0), 0), the fresh start (b = t) only when 0 is strictly greater, so
 *   a run of y_1 keeps its first frame.  State s > 0 takes the best of s, s - 1 and, for a label state with y_i != y_{i-1},
 *   s - 2, tried in that order, a candidate replacing the current best only when strictly greater.  After the max, r_t[ext_s] is
 *   added.  An unreachable state is exactly -inf with b = -1.  All arithmetic is fp32, in this order.
 * End score: (s_t, b_t) = value and start of state 2L - 2 after frame t.
 * Events: thr_abs = fp32(threshold * L) (threshold in nats per label), hold >= 1 frames.  At frame t, in this order:
 *   1. a candidate is open and t - cand.end >= hold: it is emitted and closed;
 *   2. s_t >= thr_abs and s_t > -inf: (s_t, b_t, t) opens a candidate when none is open; else it replaces the candidate when
 *      s_t > cand.score, or s_t == cand.score and b_t == cand.start (a hit extends through the run of its last label).
 *   An end (end_mask / end_all) emits an open candidate after the feed's frames.  A hit is (keyword, start, end, score).
 * Best: every (stream, keyword) tracks the largest s_t so far with (b_t, t), replaced only when strictly greater; -inf, -1, -1
 *   before any path exists.
 * lanes: the host's packing, int32 [waves * 64][4] on the device, 16-byte aligned: per lane (label, flags, keyword index,
 *   thr_abs bits).  The keywords fill waves of 64 lanes in list order, one lane per label, no keyword straddling a wave; flags:
 *   1 = the keyword's first label, 2 = its last, 4 = y_i != y_{i-1}; an unused lane has label -1.
 * state: ds2_kws_state_bytes(N, waves, K) bytes, 16-byte aligned: [N][waves][4][64] lattice words (label value, blank value,
 *   label start, blank start), [N][K][8] keyword words (candidate score, start, end; best score, start, end; two reserved; end
 *   -1 = no candidate), [N][waves] int32 frame counters (2^31 frames per stream).  ds2_kws_reset: the streams with mask[n] != 0
 *   (null = all) start again: no path, no candidate, no best, frame 0.
 * ds2_kws_feed: x is the chunk (N, Tc, C) with ds2_beam_stream_feed's strides, Tc >= 0 (0: an end alone, x may be null); sizes
 *   [N] int32 on the device (null = Tc); frames at and beyond sizes[n] are never read, and sizes[n] == 0 leaves the state of
 *   stream n bitwise as it is unless the stream ends.  Streams with end_mask[n] != 0 (device int32 [N], may be null), or all with
 *   end_all != 0, end after their frames.  out: int32 [N][ds2_kws_out_stride(K, max_hits)], 16-byte aligned: per stream the
 *   header (hits, dropped, frames consumed, 0), then the hits emitted by THIS feed as (keyword, start, end, score bits),
 *   keyword-major and in time order within a keyword.  Of one keyword's hits in one feed the first max_hits are kept and the
 *   others counted in dropped.  ws: ds2_kws_ws_bytes(N, Tc, K, max_hits) bytes, 16-byte aligned.  A one-shot call is
 *   ds2_kws_reset + one ds2_kws_feed with end_all.  Three launches (two when Tc == 0), no atomics, the same bits every time.
 * DS2_ERR_ARG: a null pointer other than sizes / mask / end_mask (x only when Tc > 0), N < 1 or > 65535, C, waves or K < 1,
 *   Tc < 0, a blank outside [0, C), a mode outside [0, 2], hold < 1, max_hits outside [1, 4096].  DS2_ERR_ALIGN as above.  Size
 *   queries: -1. */
long ds2_kws_state_bytes(int N, int waves, int K);
long ds2_kws_ws_bytes(int N, int Tc, int K, int max_hits);
long ds2_kws_out_stride(int K, int max_hits);
int ds2_kws_reset(void* state, int N, int waves, int K, const int* mask, ds2_stream_t stream);
int ds2_kws_feed(const float* x, long stride_n, long stride_t, int N, int Tc, int C, int mode, const int* sizes, int blank,
                 const int* lanes, int waves, int K, int hold, int max_hits, const int* end_mask, int end_all, void* state, int* out,
                 void* ws, ds2_stream_t stream);

/* ---- exact chunked inference: conv front-end and lookahead with carried time context -------------
 * For a uni-directional model in eval mode: fed chunk by chunk, the three kernels below give the frames of the one-shot forward.
 * Each reads, per stream n, a VIRTUAL WINDOW over time: position i < K comes from `carry` (the K positions in front of the
 * chunk), K <= i < K + len[n] from the chunk, everything else is 0; len [N] int32 on the device, null = the whole chunk; a
 * value outside [0, chunk] is clamped.  Output frame j of the call, 0 <= j < J, reads the window from position off + stride * j
 * on; frames j >= live[n] are written as zeros (live [N] int32 on the device, null = J).  Each also writes the NEXT carry
 * next[i] = V[len[n] + i], i < K, into a second buffer (next != carry: the old one is read during the call); a session
 * ping-pongs two.  A zero carry at the start of a stream is the one-shot's left zero padding.  J = 0 writes the carry alone.
 * ds2_stream_plan (host only): after `frames` input frames, a feed of `chunk` more (final != 0: the last of the utterance)
 *   computes conv1 frames [out[0], out[1]), conv2 / RNN frames [out[2], out[3]) and output frames [out[4], out[5]) -- global
 *   indices per stream, any range may be empty; out[6..8] are the `off` of conv1, conv2 and the lookahead; out[9..11] the
 *   carried positions K: 10 input frames, 10 conv1 activation frames, ctx - 1 RNN rows.  Not final, with G = frames + chunk:
 *   J1 = 0 if G < 6 else (G - 6) / 2 + 1, J2 = max(J1 - 5, 0), J3 = max(J2 - (ctx - 1), 0); final: all three (G - 1) / 2 + 1
 *   (0 for G = 0).  At the end of an utterance the per-stream totals go in through len / live.
 * ds2_stream_state_bytes (host only): the double-buffered carries of one session, each 256-byte aligned: 2 x ([N][F0][10] f32 +
 *   [N][F1][10][32] + [ctx - 1][N][H] in the storage type); 0 for an argument out of range.
 * ds2_stream_conv1: Conv2d(1, 32, (41, 11), stride (2, 2)) + eval BatchNorm2d + Hardtanh(0, 20) over [carry | x]; x [N][F0][Tc]
 *   f32, carry / next [N][F0][10] f32, K = 10, stride 2.  w1k [451][32], b1 [32] as for ds2_conv1_fwd; scale = gamma *
 *   rsqrt(running_var + eps) and shift = beta - running_mean * scale, [32] f32: y = clamp(fma(acc + bias, scale, shift), 0, 20),
 *   y [N][F1][J][32] in the storage type (what ds2_stream_conv2 reads).  Any F0 ds2_conv_rows accepts.
 * ds2_stream_conv2: Conv2d(32, 32, (21, 11), stride (2, 1)) + eval BatchNorm2d + Hardtanh(0, 20) on the matrix pipes over
 *   [carry | a1]; a1 [N][F1][Jin][32], carry / next [N][F1][10][32], w2t [21*11][32][32] in the storage type (as ds2_conv2_fwd),
 *   K = 10, stride 1.  Writes the sequence layout the recurrent stack reads: x0[(j * N + n) * rld + f * 32 + c], columns
 *   [32 * F2, rld) zero; rld >= 32 * F2, a multiple of 16; J * N * rld < 2^31.
 * ds2_stream_lookahead: y[t][n][h] = hardtanh(sum_k w[h][k] * V[off + t + k]) over rows [carry ctx - 1 | x Jin][N][H], taps
 *   ascending with fmaf (ds2_lookahead_fwd's order); w [H][ctx] f32; K = ctx - 1, stride 1; ctx = 1: no carry (null).  H a
 *   multiple of the 16-byte vector (4 f32 / 8 bf16).  No live: rows beyond a stream's end are zero already.
 * DS2_ERR_ARG: N < 1, a negative count or offset, a null buffer that the counts say is read or written, next == carry, and the
 *   limits above; DS2_ERR_DTYPE: a storage type other than f32 / bf16. */
int ds2_stream_plan(long frames, int chunk, int ctx, int final, int* out);
long ds2_stream_state_bytes(int dtype, int N, int F0, int H, int ctx);
int ds2_stream_conv1(int dtype, const float* x, const float* carry, float* next, const float* w1k, const float* b1,
                     const float* scale, const float* shift, const int* len, const int* live, void* y, int N, int F0, int Tc,
                     int off, int J, ds2_stream_t stream);
int ds2_stream_conv2(int dtype, const void* a1, const void* carry, void* next, const void* w2t, const float* b2, const float* scale,
                     const float* shift, const int* len, const int* live, void* x0, int N, int F0, int Jin, int off, int J,
                     int rld, ds2_stream_t stream);
int ds2_stream_lookahead(int dtype, const void* x, const void* carry, void* next, const float* w, const int* len, void* y, int N,
                         int H, int ctx, int Jin, int off, int J, ds2_stream_t stream);

/* ---- exact chunked inference for a pool of streams that start and end on their own ---------------
 * The same three kernels with one ds2_stream_row per batch row instead of one off / J for the batch: every stream follows its
 * own ds2_stream_plan, and a feed may hold any subset of the pool's S slots.  rows: [n_rows] on the device.  The carries of a
 * stage are two buffers over all S slots, carry0 / carry1, in ds2_stream_state_bytes' layouts with N = S; bit s - 1 of `cur`
 * says which of the two holds the slot's carry of stage s (1 = conv1, 2 = conv2, 3 = lookahead): the call reads that buffer's
 * slot and writes the other one's, so the caller flips the bit of every row of a launched stage, and slots that are not in
 * `rows` keep both buffers as they are.  Bit s - 1 of `fresh` makes the carry of stage s read as zero whatever the buffer holds
 * (a stream's feeds until that stage has written its first carry).
 * The window of stage s for row r is [carry K | the row's new positions], zero beyond: len input frames for conv1, cnt1 conv1
 * activations for conv2, cnt2 RNN rows for the lookahead (each clamped to the launch's Tc / Jin).  Output frame j < cnt_s reads
 * it from off_s + stride * j on, frames cnt_s <= j < J are written as zeros, J >= every row's cnt_s.  The next carry is
 * V[new positions + i], i < K: a plain copy for a row with nothing new.
 * ds2_stream_conv1_rows: x is the caller's tensor [.][F0][Tc], row r reads x[src]; y [n_rows][F1][J][32] in table order.
 * ds2_stream_conv2_rows: a1 [n_rows][F1][Jin][32] (conv1_rows' y); x0[(j * n_rnn + r) * rld + ...] for the rows r < n_rnn,
 *   which must be the rows with cnt2 > 0 (the table is ordered by cnt2 descending, what the recurrent stack takes); the rows
 *   behind them only move their carry.  J = 0 exactly when n_rnn = 0.
 * ds2_stream_lookahead_rows: x [Jin][n_rnn][H] and y [J][n_rnn][H] over the first n_rnn rows of the table; S is the slot
 *   count of the carry buffers [ctx - 1][S][H].
 * The table lives on the device, so the entries cannot check it: slot must lie in [0, S) and be distinct over the rows, src
 * inside x, offsets >= 0 (ops.stream_rows checks them on the host).  Otherwise the arguments, limits and errors are those above. */
typedef struct ds2_stream_row {
  int32_t slot;        /* the stream's carry slot, 0 <= slot < S */
  int32_t src;         /* the stream's row of x in the caller's tensor */
  int32_t cur;         /* bit s - 1: the buffer that holds the carry of stage s */
  int32_t fresh;       /* bit s - 1: the carry of stage s reads as zero */
  int32_t len;         /* input frames of the row's chunk */
  int32_t off1, cnt1;  /* conv1: window offset and output frames */
  int32_t off2, cnt2;  /* conv2 (= RNN frames) */
  int32_t off3, cnt3;  /* lookahead (= output frames) */
  int32_t reserved[5]; /* 64 bytes a row */
} ds2_stream_row;
int ds2_stream_conv1_rows(int dtype, const float* x, float* carry0, float* carry1, const ds2_stream_row* rows, const float* w1k,
                          const float* b1, const float* scale, const float* shift, void* y, int n_rows, int F0, int Tc, int J,
                          ds2_stream_t stream);
int ds2_stream_conv2_rows(int dtype, const void* a1, void* carry0, void* carry1, const ds2_stream_row* rows, const void* w2t,
                          const float* b2, const float* scale, const float* shift, void* x0, int n_rows, int n_rnn, int F0, int Jin,
                          int J, int rld, ds2_stream_t stream);
int ds2_stream_lookahead_rows(int dtype, const void* x, void* carry0, void* carry1, const ds2_stream_row* rows, const float* w, void* y,
                              int n_rnn, int S, int H, int ctx, int Jin, int J, ds2_stream_t stream);

/* ---- character / word error counts on the device (the edit distances of validation.py:66-132, decoder.CharErrorRate /
 * WordErrorRate) ----
 * hyp: P rows of int32 labels, row p at hyp + p * hyp_stride with hyp_lens[p] labels; ref: the references' labels back to back,
 * reference r = ref[ref_offsets[r] .. ref_offsets[r + 1]), ref_offsets [R + 1] int32.  Pair p compares hypothesis p with reference
 * p % R (the [G][N] rows of ds2_beam_decode_lm_grid against N references).  All pointers are device memory; labels are >= 0.
 *   char_err [P]: Levenshtein distance of the label strings without the space label; ref_chars [R]: the reference's length without it
 *   word_err [P]: Levenshtein distance over words (maximal runs of non-space labels, identified by the beam search's 61-bit string
 *                 hash); ref_words [R]: the reference's number of words
 * A string may have up to 4096 labels.  The lengths live on the device, so the entry cannot refuse a longer one: the kernel reads
 * nothing of such a pair and writes -1 to its outputs (ops.error_counts checks the lengths and raises).
 * DS2_ERR_ARG: P < 1, R < 1, R > P, hyp_stride < 0, a null pointer. */
int ds2_error_counts(const int* hyp, long hyp_stride, const int* hyp_lens, int P, const int* ref, const int* ref_offsets, int R,
                     int space, int* char_err, int* word_err, int* ref_chars, int* ref_words, ds2_stream_t stream);

/* ---- CTC forced alignment on the device: the best (Viterbi) path of a KNOWN transcript and per-label frame spans --------------
 * x[n*stride_n + t*stride_t + c] f32, addressed as the decoders address it; mode 0: logits (log-softmax over the C classes in fp32,
 * with ds2_ctc_loss_grad's summation order), 1: probabilities (logf; a probability of 0 is -inf), 2: log-probabilities as they
 * are.  sizes [N] int32 on the device (null = Tp); targets / target_offsets / target_lengths as for ds2_ctc_loss_grad.
 * Lattice over ext[2i] = blank, ext[2i+1] = target[i] (S = 2L + 1 states), fp32, unreachable states exactly -inf:
 *   v[0][0] = lp[0][blank], v[0][1] = lp[0][ext[1]];  v[t][s] = lp[t][ext[s]] + max(v[t-1][s], v[t-1][s-1], v[t-1][s-2]),
 *   the s-2 predecessor only when ext[s] is a label that differs from ext[s-2].
 * Tie rule: among equal predecessors s, then s-1, then s-2; at the end an equal value goes to state 2L rather than 2L - 1.
 * Outputs (device; EVERY element is written on every call):
 *   frame_state [N][Tp] int32: the lattice state of every frame (label index = state >> 1 for an odd state, blank for an even
 *                 one); -1 for t >= sizes[n] and for a clip without a path
 *   tok_start / tok_end (flat like targets) int32: first / last frame (inclusive) of every label; tok_logp f32: the sum of the
 *                 label's frame log-probabilities in increasing frame order
 *   score [N] f32: log-probability of the best path; -inf when no path exists (sizes[n] = 0, fewer frames than labels plus
 *                 adjacent equal labels, a best value of -inf, a label outside [0, C)): then the clip's frame_state, tok_start and
 *                 tok_end are -1 and its tok_logp 0.
 * max_target_len: at least max over target_lengths, at most 2047.  A clip whose target_lengths[n] lies outside
 * [0, max_target_len] gets score -inf and frame_state -1 and its tok entries are NOT touched (the length cannot be trusted).
 * ws: ds2_ctc_align_ws_bytes(Tp, N, max_target_len) bytes, 4-byte aligned ([N][Tp] f32 log-normalisers, then one back-pointer
 * byte per (n, t, state) with a row stride of 2 max_target_len + 1 rounded up to 4); -1 for arguments ds2_ctc_align refuses.
 * Same bits on every launch.  DS2_ERR_ARG: N, Tp or C < 1, blank outside [0, C), mode outside [0, 2], max_target_len outside
 * [0, 2047], a null pointer other than sizes. */
long ds2_ctc_align_ws_bytes(int Tp, int N, int max_target_len);
int ds2_ctc_align(const float* x, long stride_n, long stride_t, int N, int Tp, int C, int mode, const int* sizes, const int* targets,
                  const int* target_offsets, const int* target_lengths, int max_target_len, int blank, int* frame_state,
                  int* tok_start, int* tok_end, float* tok_logp, float* score, void* ws, ds2_stream_t stream);

/* ---- word timings and confidence of hypotheses a CTC decoder returned ---------------------------------
 * x, stride_n, stride_t, sizes as for ds2_ctc_align; kind 0: logits, 1: probabilities, 2: log-probabilities.  Frame t of row n is
 * read at row (t0[n] + t) mod cap of x (t0 [N] int32 on the device, null = 0; cap >= Tp; a one-shot call passes null and Tp).
 * Hypothesis (n, b), b < B: lens[n*B + b] labels tokens[(n*B + b)*ld + i] at frames offsets[...], as the decoders return them.
 * A hypothesis with a length outside [0, ld], a label outside [0, C) or a frame outside [0, sizes[n]) is used as no index and
 * comes back INVALID: every confidence NaN, every span and word entry -1, 0 words.
 * Frame pass, for every valid frame: p_t(c), an fp32 number: the value as given (probabilities, not renormalised),
 * exp(x - lz) (logits) or exp(x) (log-probabilities), evaluated in fp64 and rounded once; lz = m + log(sum exp(x - m)), m the
 * frame's maximum, in fp64 rounded once to fp32.  a_t: the first maximal class by the greedy decoder's scan (class 0 wins when it
 * is NaN, a NaN elsewhere never wins).  m_t, the frame value of `measure`, V = C:
 *   0 label_prob  none: a token uses p_t(l) of its own label l        1 max_prob  p_t(a_t)
 *   2 entropy     1 - H / ln V, H = -sum p ln p (a zero term is 0)
 *   3 tsallis     1 - H / Hmax, H = (1 - sum p^alpha) / (alpha - 1), Hmax = (1 - V^(1 - alpha)) / (alpha - 1)
 *   4 renyi       1 - H / ln V, H = ln(sum p^alpha) / (1 - alpha)
 * 2 to 4 in fp64, clamped to [0, 1], rounded once.  SUMMATION ORDER of every sum over the classes (lz's too): 64 partial sums, the
 * j-th over the classes j, j + 64, ... in increasing order, then v[j] += v[j ^ o] for o = 32, 16, 8, 4, 2, 1.
 * Token i (label l, frame o): forward end e_i: from o, t = o + 1, ... while t < sizes[n], a_t == l and t < offsets[i + 1] (if
 * there is a next token); start s_i: t = o - 1, ... while t >= 0, a_t == l and t > e_(i-1) (if there is a previous token).  The
 * span [s_i, e_i] always holds o.  tok_conf = aggregate (0 mean, 1 min, 2 prod) of m_t, or p_t(l), over the span in increasing
 * frame order: fp64 sum / count or product, rounded once; min is exact.  The space label is a token like any other.
 * Words: maximal runs of tokens other than `space` (space = any value >= C: one word).  word_first / word_last: token indices;
 * word_start = s_first, word_end = e_last; word_conf = word_aggregate over the tokens' fp32 confidences in order; utt_conf =
 * word_aggregate over the word confidences, NaN without words.
 * Outputs (device; EVERY element is written on every call; entries past a length or a count are -1 / NaN):
 *   tok_start, tok_end int32 and tok_conf f32 [N][B][ld]; word_first, word_last, word_start, word_end int32 and word_conf f32
 *   [N][B][lw], 2 lw >= ld; word_count int32 and utt_conf f32 [N][B].
 * ws: ds2_confidence_ws_bytes(N, Tp) bytes, 4-byte aligned (a_t, m_t, lz: 12 bytes per frame); -1 for N or Tp < 1.
 * No atomics; the same bits on every launch.  DS2_ERR_ARG: N outside [1, 65535], Tp, ld < 1, N * Tp > 2^31 - 1, C outside [1, 8192] (entropy
 * measures: [2, 8192]), B outside [1, 256], 2 lw < ld, cap < Tp, blank outside [0, C), space < 0, kind, measure or an aggregate
 * out of range, alpha <= 0 or == 1 for measures 3 and 4, a null pointer other than sizes and t0. */
long ds2_confidence_ws_bytes(int N, int Tp);
int ds2_confidence(const float* x, long stride_n, long stride_t, int N, int Tp, int C, int kind, const int* sizes, const int* t0,
                   int cap, const int* tokens, const int* offsets, const int* lens, int B, int ld, int lw, int blank, int space,
                   int measure, double alpha, int aggregate, int word_aggregate, int* tok_start, int* tok_end, float* tok_conf,
                   int* word_first, int* word_last, int* word_start, int* word_end, float* word_conf, int* word_count,
                   float* utt_conf, void* ws, ds2_stream_t stream);
/* A stream keeps its frames for ds2_confidence: row j < sizes[n] of chunk x [N][Tc][C] goes to row (count[n] + j) mod cap of
 * store [N][cap][C] f32, then count[n] += sizes[n]; sizes (null = Tc) and count [N] int32 are read on the device, so a feed waits
 * for nothing.  DS2_ERR_ARG: N outside [1, 65535], Tc < 1, C outside [1, 8192], cap < Tc, a null pointer other than sizes. */
int ds2_frame_store_append(const float* x, long stride_n, long stride_t, int N, int Tc, int C, const int* sizes, int* count,
                           float* store, int cap, ds2_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* DS2HIP_H */
