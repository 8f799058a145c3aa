// Log-spectrogram front-end on the device: what SpectrogramParser.compute_spectrogram does per
// utterance on the CPU loader workers (reference loader/data_loader.py:73-94: librosa.stft(n_fft = win_length = 320, hop 160,
// hamming window, center = True) -> magnitude -> log1p -> (x - mean) / std over the whole utterance) and what _collate_fn does
// with the results (:247-270: zero-padded (N, 1, 161, Tmax) batch), producing the model's input tensor directly.
//
// The 320-point real DFT of every frame is one fp32 MFMA GEMM: the frames of an utterance are the rows of a matrix with row
// stride = hop (overlapping rows of the centre-padded waveform, no frame copy), the basis [2*161][320] carries the window.
//   k_spect_pad   : waveform -> centre-padded copy (zeros = librosa >= 0.10 default, or reflect = older default: np.pad's
//                   "reflect", which keeps folding when the clip is shorter than the 160-sample pad)
//   ds2_gemm_nt   : C[t][0:161] = Re, C[t][161:322] = Im      (v_mfma_f32_32x32x2_f32, exact fp32 products)
//   k_spect_stats : per utterance sum / sum of squares of log1p(|X|) over its own frames (fp64 partials, fixed order)
//   k_spect_write : normalise, transpose to [f][t] through LDS, zero the padding frames
// SpecAugment (reference loader/spec_augment.py:48-115, `augmentation.spec_augment: True` of its LibriSpeech / TED-LIUM / Common
// Voice configurations) rides on the same pass:
//   k_spect_warp_coef    : per clip, the three coefficients of the affine time flow that the reference's one-control-point
//                          sparse_image_warp produces (fp64; reads the control value from the GEMM output, nothing visits the host)
//   k_spect_write<true>  : the write kernel with the warp (two source frames, linear interpolation) and the masks folded in
//   k_spec_augment       : the same warp + masks over an existing (N, 1, F, Tmax) batch, any F
// Roofline: MFMA fp32 (2*320*322 flop per frame) against ~1.3 KB of HBM traffic per frame: compute-bound on the fp32 matrix
// pipe (157 TFLOP/s), ~0.1 ms for a 32 x 15 s batch; the CPU path spends tens of ms per clip.
#include "ds2_common.h"

extern "C" int ds2_gemm_nt(int dtype, const void* A, const void* B, void* C, const float* bias, int M, int N, int K, long lda,
                           long ldb, long ldc, int out_f32, int batch, long strideA, long strideB, long strideC, long strideBias,
                           int splitk, ds2_stream_t st);

namespace {

constexpr int NFFT = 320, HOP = 160, NBIN = 161, LDC = 336;   // LDC: row stride of the GEMM output (322 rounded up to 16)
constexpr int STAT_BLOCKS = 32;

__global__ void __launch_bounds__(256) k_spect_pad(const float* __restrict__ wav, long ldw, const int* __restrict__ nsamp, int reflect,
                                                   float* __restrict__ ypad, long lpad) {
  const int n = blockIdx.y;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= lpad) return;
  const int L = nsamp[n];
  long s = i - NFFT / 2;
  float v = 0.f;
  if (i < (long)L + NFFT) {              // inside this utterance's padded extent
    if (reflect && (s < 0 || s >= L)) {  // np.pad(mode = "reflect"): fold with period 2 (L - 1) as often as a short clip needs
      const long p = 2 * ((long)L - 1);
      if (p == 0) {
        s = 0;                           // a single sample repeats
      } else {
        s %= p;
        if (s < 0) s += p;
        if (s >= L) s = p - s;
      }
    }
    if (s >= 0 && s < L) v = wav[(long)n * ldw + s];
  }
  ypad[(long)n * lpad + i] = v;
}

__device__ __forceinline__ float logmag(const float* row, int f) {
  const float re = row[f], im = row[NBIN + f];
  return log1pf(sqrtf(re * re + im * im));
}

// grid (STAT_BLOCKS, N): block b of sample n sums its share of the frames
__global__ void __launch_bounds__(256) k_spect_stats(const float* __restrict__ C, long strideC, const int* __restrict__ nsamp,
                                                     double* __restrict__ partial) {
  __shared__ double red[2][4];
  const int n = blockIdx.y;
  const int T = 1 + nsamp[n] / HOP;
  const float* Cn = C + (long)n * strideC;
  double s = 0.0, q = 0.0;
  for (int t = blockIdx.x; t < T; t += STAT_BLOCKS) {
    const float* row = Cn + (long)t * LDC;
    if (threadIdx.x < NBIN) {
      const double v = (double)logmag(row, threadIdx.x);
      s += v;
      q += v * v;
    }
  }
  for (int o = 32; o > 0; o >>= 1) {
    s += __shfl_xor(s, o, 64);
    q += __shfl_xor(q, o, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    red[0][threadIdx.x >> 6] = s;
    red[1][threadIdx.x >> 6] = q;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    partial[((long)n * STAT_BLOCKS + blockIdx.x) * 2] = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
    partial[((long)n * STAT_BLOCKS + blockIdx.x) * 2 + 1] = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
  }
}

// mean / 1/std per sample: torch's spect.mean() and spect.std() (unbiased, data_loader.py:88-92)
__global__ void k_spect_finalize(const double* __restrict__ partial, const int* __restrict__ nsamp, int N, float* __restrict__ ms) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  double s = 0.0, q = 0.0;
  for (int b = 0; b < STAT_BLOCKS; ++b) {
    s += partial[((long)n * STAT_BLOCKS + b) * 2];
    q += partial[((long)n * STAT_BLOCKS + b) * 2 + 1];
  }
  const double cnt = (double)NBIN * (1 + nsamp[n] / HOP);
  const double mean = s / cnt;
  double var = (q - cnt * mean * mean) / (cnt - 1.0);
  if (var < 0.0) var = 0.0;
  ms[2 * n] = (float)mean;
  ms[2 * n + 1] = (float)(1.0 / sqrt(var));
}

// ---- SpecAugment ---------------------------------------------------------------------------------------------------------
constexpr int MAX_MASKS = 4;

struct AugArgs {            // per-clip augmentation inputs of the write kernel (unused by the plain instantiation)
  const float* coef;        // [N][3] (a_f, a_t, a_0): flow_t(f, t) = a_f f + a_t t + a_0; all zero = no warp
  const int* fmask;         // [N][MF][2] start, width
  const int* tmask;         // [N][MT][2]
  int MF, MT;
};

// a cell inside one of the M [start, start + width) intervals (width <= 0: no mask)
__device__ __forceinline__ bool aug_masked(const int* __restrict__ m, int M, int p) {
  bool z = false;
  for (int k = 0; k < M; ++k) {
    const int s = m[2 * k], w = m[2 * k + 1];
    z |= w > 0 && p >= s && (long)p < (long)s + w;
  }
  return z;
}

// source frame pair and weight of output (f, t): q = t - flow_t(f, t), fl = clamp(floor(q), 0, T - 2), alpha = clamp(q - fl, 0, 1)
// (interpolate_bilinear, sparse_image_warp.py:357-408).  alpha is taken as (t - fl) - flow, which rounds once at the size of the
// flow and not at the size of t.  fminf / fmaxf drop a NaN operand, so a non-finite flow still yields 0 <= fl <= T - 2.  T >= 2.
__device__ __forceinline__ void aug_source(float af, float at, float a0, int f, int t, int T, int& fl, float& alpha) {
  const float flow = fmaf(af, (float)f, fmaf(at, (float)t, a0));
  const float flf = fminf(fmaxf(floorf((float)t - flow), 0.f), (float)(T - 2));
  fl = (int)flf;
  alpha = fminf(fmaxf(((float)t - flf) - flow, 0.f), 1.f);
}

__device__ __forceinline__ float aug_lerp(float lo, float hi, float alpha) { return fmaf(alpha, hi - lo, lo); }   // :406

// One thread per clip, fp64.  draw [N][12] f32: frame index i, shift d, the 3 x 3 block E (randn / 1e10, row major), one pad.
// The reference's system for its single control point c = (F/2, pt + d, 1), pt = spect[F/2][i]  (spec_augment.py:56-62,
// sparse_image_warp.py:141-184) is [[0, c^T], [c, E]] (w; v) = (d; 0):  v = d adj(E) c / (c^T adj(E) c) (det E cancels),
// w = -d det(E) / (c^T adj(E) c).  The radial term w * phi(r) is evaluated by the reference at r = S - 2 q.c + |c|^2 with S the sum
// of the squared norms of ALL grid points (:197-198), i.e. the constant K = w * phi(S + |c|^2).  coef = (v_0, v_1, v_2 + K).
// GEMM: pt comes from the front-end's GEMM output (normalised as the write kernel normalises); else from a batch (N, 1, F, ld).
// Zero coefficients (= no warp): null draw, i < 0 or i >= T, T <= 2W (the reference's randrange raises there), non-finite result.
template <bool GEMM>
__global__ void k_spect_warp_coef(const float* __restrict__ src, long strideN, int ld, const int* __restrict__ len,
                                  const float* __restrict__ ms, int normalize, const float* __restrict__ draw, int N, int F, int W,
                                  float* __restrict__ coef, float* __restrict__ coef_out) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  double a[3] = {0.0, 0.0, 0.0};
  int T = GEMM ? 1 + len[n] / HOP : len[n];
  if (!GEMM && T > ld) T = ld;
  const int i = draw ? (int)draw[12 * n] : -1;
  if (i >= 0 && i < T && T > 2 * W) {
    const float* dr = draw + 12 * n;
    const float d = dr[1];
    float pt;
    if (GEMM) {
      const float mean = normalize ? ms[2 * n] : 0.f, rstd = normalize ? ms[2 * n + 1] : 1.f;
      pt = (logmag(src + n * strideN + (long)i * LDC, F / 2) - mean) * rstd;
    } else {
      pt = src[n * strideN + (long)(F / 2) * ld + i];
    }
    const double c[3] = {(double)(F / 2), (double)(pt + d), 1.0};          // the reference holds c in fp32
    double E[9];
    for (int k = 0; k < 9; ++k) E[k] = (double)dr[2 + k];
    const double adj[9] = {E[4] * E[8] - E[5] * E[7], E[2] * E[7] - E[1] * E[8], E[1] * E[5] - E[2] * E[4],
                           E[5] * E[6] - E[3] * E[8], E[0] * E[8] - E[2] * E[6], E[2] * E[3] - E[0] * E[5],
                           E[3] * E[7] - E[4] * E[6], E[1] * E[6] - E[0] * E[7], E[0] * E[4] - E[1] * E[3]};
    const double det = E[0] * adj[0] + E[1] * adj[3] + E[2] * adj[6];
    double u[3], q = 0.0;
    for (int r = 0; r < 3; ++r) {
      u[r] = adj[3 * r] * c[0] + adj[3 * r + 1] * c[1] + adj[3 * r + 2] * c[2];
      q += c[r] * u[r];
    }
    const double Fd = F, Td = T;
    const double S = Td * ((Fd - 1) * Fd * (2 * Fd - 1) / 6) + Fd * ((Td - 1) * Td * (2 * Td - 1) / 6) + c[0] * c[0] + c[1] * c[1];
    const double K = (-(double)d * det / q) * (0.5 * S * log(S));          // S >= 1: the reference's max(r, 1e-10) never binds
    a[0] = d * u[0] / q;
    a[1] = d * u[1] / q;
    a[2] = d * u[2] / q + K;
    if (!(isfinite(a[0]) && isfinite(a[1]) && isfinite(a[2]))) a[0] = a[1] = a[2] = 0.0;
  }
  for (int k = 0; k < 3; ++k) {
    coef[3 * n + k] = (float)a[k];
    if (coef_out) coef_out[3 * n + k] = (float)a[k];
  }
}

// grid (ceil(Tmax/64), 3, N): 64 frames x 64 bins per block through LDS; out[n][0][f][t].  AUG: every output takes its value
// from the clip's own frames fl, fl + 1 <= T - 1 (rows of the GEMM output are [t][LDC]: a wave reads 64 neighbouring bins of one
// or two rows, the transpose tile keeps the stores coalesced) and masked cells are written as 0.
template <bool AUG>
__global__ void __launch_bounds__(256) k_spect_write(const float* __restrict__ C, long strideC, const int* __restrict__ nsamp,
                                                     const float* __restrict__ ms, int normalize, float* __restrict__ out, int Tmax,
                                                     AugArgs aug) {
  __shared__ float tile[64][65];
  const int n = blockIdx.z, t0 = blockIdx.x * 64, f0 = blockIdx.y * 64;
  const int T = 1 + nsamp[n] / HOP;
  const float mean = normalize ? ms[2 * n] : 0.f, rstd = normalize ? ms[2 * n + 1] : 1.f;
  const float* Cn = C + (long)n * strideC;
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  float af = 0.f, at = 0.f, a0 = 0.f;
  bool warp = false, fz = false;
  const int* tm = nullptr;
  if constexpr (AUG) {
    af = aug.coef[3 * n], at = aug.coef[3 * n + 1], a0 = aug.coef[3 * n + 2];
    warp = (af != 0.f || at != 0.f || a0 != 0.f) && T >= 2;
    fz = aug_masked(aug.fmask + (long)n * aug.MF * 2, aug.MF, f0 + tx);
    tm = aug.tmask + (long)n * aug.MT * 2;
  }
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int t = t0 + ty * 16 + i, f = f0 + tx;
    float v = 0.f;
    if (t < T && f < NBIN) {
      if constexpr (AUG) {
        if (fz || aug_masked(tm, aug.MT, t)) {
          v = 0.f;
        } else if (warp) {
          int fl;
          float alpha;
          aug_source(af, at, a0, f, t, T, fl, alpha);
          const float lo = (logmag(Cn + (long)fl * LDC, f) - mean) * rstd, hi = (logmag(Cn + (long)(fl + 1) * LDC, f) - mean) * rstd;
          v = aug_lerp(lo, hi, alpha);
        } else {
          v = (logmag(Cn + (long)t * LDC, f) - mean) * rstd;
        }
      } else {
        v = (logmag(Cn + (long)t * LDC, f) - mean) * rstd;
      }
    }
    tile[ty * 16 + i][tx] = v;
  }
  __syncthreads();
  float* on = out + (long)n * NBIN * Tmax;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int f = f0 + ty * 16 + i, t = t0 + tx;
    if (f < NBIN && t < Tmax) on[(long)f * Tmax + t] = tile[tx][ty * 16 + i];
  }
}

// grid (ceil(Tmax/256), F, N): x, y (N, 1, F, Tmax); consecutive threads take consecutive t of one row, so the two gathered
// source frames of a wave are a contiguous stretch of that row (|d fl / d t| = |1 - a_t|) and the stores are coalesced.
__global__ void __launch_bounds__(256) k_spec_augment(const float* __restrict__ x, float* __restrict__ y, int F, int Tmax,
                                                      const int* __restrict__ frames, AugArgs aug) {
  const int n = blockIdx.z, f = blockIdx.y, t = blockIdx.x * 256 + threadIdx.x;
  if (t >= Tmax) return;
  const int T = min(max(frames[n], 0), Tmax);
  const float af = aug.coef[3 * n], at = aug.coef[3 * n + 1], a0 = aug.coef[3 * n + 2];
  const float* row = x + ((long)n * F + f) * Tmax;
  float v = 0.f;
  if (t < T && !aug_masked(aug.fmask + (long)n * aug.MF * 2, aug.MF, f) && !aug_masked(aug.tmask + (long)n * aug.MT * 2, aug.MT, t)) {
    if ((af != 0.f || at != 0.f || a0 != 0.f) && T >= 2) {
      int fl;
      float alpha;
      aug_source(af, at, a0, f, t, T, fl, alpha);
      v = aug_lerp(row[fl], row[fl + 1], alpha);
    } else {
      v = row[t];
    }
  }
  y[((long)n * F + f) * Tmax + t] = v;
}

inline long pad_len(int Lmax) { return (((long)Lmax + NFFT + 3) / 4) * 4 + NFFT; }

}  // namespace

extern "C" {

// frames of a waveform of `nsamples` samples (librosa.stft, center = True): 1 + nsamples / hop
int ds2_spect_frames(int nsamples) { return 1 + nsamples / HOP; }
// bytes of scratch: padded waveforms + GEMM output + statistics + warp coefficients
long ds2_spect_ws_bytes(int N, int Lmax) {
  const long Tmax = 1 + Lmax / HOP;
  return ((long)N * pad_len(Lmax) + (long)N * Tmax * LDC + 2L * N + 16) * 4 + (long)N * STAT_BLOCKS * 2 * 8 + 4L * N * 4;
}

namespace {

// the shared body of ds2_spectrogram / ds2_spectrogram_aug: aug == nullptr launches the plain write kernel
int spectrogram_impl(const float* wav, long ldw, const int* nsamples, int N, int Lmax, const float* basis, int reflect,
                     int normalize, float* out, void* ws, const float* warp_draw, int W, const AugArgs* aug, float* coef_out,
                     hipStream_t st) {
  const long lpad = pad_len(Lmax);
  const int Tmax = 1 + Lmax / HOP;
  float* ypad = (float*)ws;
  float* Cbuf = ypad + (long)N * lpad;
  float* ms = Cbuf + (long)N * Tmax * LDC;
  double* partial = (double*)(((uintptr_t)(ms + 2L * N) + 15) & ~(uintptr_t)15);
  float* coef = (float*)(partial + (long)N * STAT_BLOCKS * 2);
  hipLaunchKernelGGL(k_spect_pad, dim3(ds2_cdiv(lpad, 256), N), dim3(256), 0, st, wav, ldw, nsamples, reflect, ypad, lpad);
  DS2_CHECK_LAUNCH();
  int rc = ds2_gemm_nt(DS2_F32, ypad, basis, Cbuf, nullptr, Tmax, 2 * NBIN, NFFT, HOP, NFFT, LDC, 1, N, lpad, 0, (long)Tmax * LDC, 0, 1,
                       (ds2_stream_t)st);
  if (rc != 0) return rc;
  if (normalize) {
    hipLaunchKernelGGL(k_spect_stats, dim3(STAT_BLOCKS, N), dim3(256), 0, st, (const float*)Cbuf, (long)Tmax * LDC, nsamples, partial);
    DS2_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_spect_finalize, dim3(ds2_cdiv(N, 64)), dim3(64), 0, st, (const double*)partial, nsamples, N, ms);
    DS2_CHECK_LAUNCH();
  }
  const dim3 grid(ds2_cdiv(Tmax, 64), 3, N);
  if (!aug) {
    hipLaunchKernelGGL(k_spect_write<false>, grid, dim3(256), 0, st, (const float*)Cbuf, (long)Tmax * LDC, nsamples, (const float*)ms,
                       normalize, out, Tmax, AugArgs{});
    DS2_CHECK_LAUNCH();
    return 0;
  }
  hipLaunchKernelGGL(k_spect_warp_coef<true>, dim3(ds2_cdiv(N, 64)), dim3(64), 0, st, (const float*)Cbuf, (long)Tmax * LDC, Tmax,
                     nsamples, (const float*)ms, normalize, warp_draw, N, NBIN, W, coef, coef_out);
  DS2_CHECK_LAUNCH();
  AugArgs a = *aug;
  a.coef = coef;
  hipLaunchKernelGGL(k_spect_write<true>, grid, dim3(256), 0, st, (const float*)Cbuf, (long)Tmax * LDC, nsamples, (const float*)ms,
                     normalize, out, Tmax, a);
  DS2_CHECK_LAUNCH();
  return 0;
}

}  // namespace

// wav [N][ldw] f32 (utterance n = first nsamples[n] entries of row n), nsamples [N] device int32, 16 kHz / 20 ms / 10 ms
// geometry (n_fft 320, hop 160: the geometry the conv kernels are specialised for).  basis [322][320] f32: rows 0..160
// window[k] * cos(2 pi f k / 320), rows 161..321 -window[k] * sin(...) (built by the binding, any window).  reflect: 0 =
// zero centre padding, 1 = reflect.  normalize: (x - mean) / std per utterance (unbiased std, as torch .std()).
// out (N, 1, 161, Tmax) f32 with Tmax = 1 + Lmax/160, frames >= the utterance's own count are zero (_collate_fn layout).
int ds2_spectrogram(const float* wav, long ldw, const int* nsamples, int N, int Lmax, const float* basis, int reflect,
                    int normalize, float* out, void* ws, ds2_stream_t st_) {
  DS2_REQUIRE(wav && nsamples && basis && out && ws && N > 0 && Lmax > 0 && ldw >= Lmax, DS2_ERR_ARG);
  return spectrogram_impl(wav, ldw, nsamples, N, Lmax, basis, reflect, normalize, out, ws, nullptr, 0, nullptr, nullptr, (hipStream_t)st_);
}

// ds2_spectrogram followed by the reference's spec_augment on every clip (loader/spec_augment.py:68-115: time_warp(spec) with its
// default W, :48-65 -> sparse_image_warp, loader/sparse_image_warp.py:88-111, then frequency and time masks, :98-113), applied as
// the reference applies it: to the clip's own normalised F x T spectrogram, before the batch is padded.  warp_draw [N][12] f32 on
// the device (null = no warp): frame index i (randrange(W, T - W); negative = no warp for that clip), shift d (randrange(-W, W)),
// the nine values of randn(3, 3) / 1e10 (sparse_image_warp.py:170), one pad.  fmask [N][MF][2] / tmask [N][MT][2] int32 = start
// and width of each mask (width <= 0: none), MF, MT <= 4, null iff the count is 0.  A clip with T <= 2W frames is not warped (the
// reference raises ValueError from randrange).  coef_out (optional) [N][3] f32: the flow coefficients (a_f, a_t, a_0) used.
int ds2_spectrogram_aug(const float* wav, long ldw, const int* nsamples, int N, int Lmax, const float* basis, int reflect,
                        int normalize, float* out, void* ws, const float* warp_draw, int W, const int* fmask, int MF,
                        const int* tmask, int MT, float* coef_out, ds2_stream_t st_) {
  DS2_REQUIRE(wav && nsamples && basis && out && ws && N > 0 && Lmax > 0 && ldw >= Lmax, DS2_ERR_ARG);
  DS2_REQUIRE(W >= 0 && MF >= 0 && MF <= MAX_MASKS && MT >= 0 && MT <= MAX_MASKS && (fmask || MF == 0) && (tmask || MT == 0), DS2_ERR_ARG);
  const AugArgs a{nullptr, fmask, tmask, MF, MT};
  return spectrogram_impl(wav, ldw, nsamples, N, Lmax, basis, reflect, normalize, out, ws, warp_draw, W, &a, coef_out, (hipStream_t)st_);
}

// The flow coefficients of the reference's time warp (spec_augment.py:48-65, sparse_image_warp.py:132-184, 236-266) for a batch
// x (N, 1, F, Tmax) f32 that exists already: frames [N] device int32, warp_draw as above, coef [N][3] f32 out.
int ds2_spec_augment_coef(const float* x, int N, int F, int Tmax, const int* frames, const float* warp_draw, int W, float* coef,
                          ds2_stream_t st_) {
  hipStream_t st = (hipStream_t)st_;
  DS2_REQUIRE(x && frames && coef && N > 0 && F > 0 && Tmax > 0 && W >= 0, DS2_ERR_ARG);
  hipLaunchKernelGGL(k_spect_warp_coef<false>, dim3(ds2_cdiv(N, 64)), dim3(64), 0, st, x, (long)F * Tmax, Tmax, frames,
                     (const float*)nullptr, 0, warp_draw, N, F, W, coef, (float*)nullptr);
  DS2_CHECK_LAUNCH();
  return 0;
}

// The warp and masks of spec_augment (spec_augment.py:94-113; dense_image_warp / interpolate_bilinear, sparse_image_warp.py:
// 269-410) on a batch in (N, 1, F, Tmax) f32 -> out (same shape, out != in), any F: clip n is its first frames[n] frames (device
// int32), coef [N][3] f32 its flow coefficients (all zero = no warp), masks as in ds2_spectrogram_aug.  Frames >= frames[n] of out
// are zero.
int ds2_spec_augment(const float* in, float* out, int N, int F, int Tmax, const int* frames, const float* coef, const int* fmask,
                     int MF, const int* tmask, int MT, ds2_stream_t st_) {
  hipStream_t st = (hipStream_t)st_;
  DS2_REQUIRE(in && out && in != out && frames && coef && N > 0 && N <= 65535 && F > 0 && F <= 65535 && Tmax > 0, DS2_ERR_ARG);
  DS2_REQUIRE(MF >= 0 && MF <= MAX_MASKS && MT >= 0 && MT <= MAX_MASKS && (fmask || MF == 0) && (tmask || MT == 0), DS2_ERR_ARG);
  hipLaunchKernelGGL(k_spec_augment, dim3(ds2_cdiv(Tmax, 256), F, N), dim3(256), 0, st, in, out, F, Tmax, frames,
                     AugArgs{coef, fmask, tmask, MF, MT});
  DS2_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
