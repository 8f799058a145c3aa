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
// Running (causal) normalisation, normalize = 2: frame t is normalised with the mean and the standard
// deviation of frames 0..t, so nothing depends on audio that has not arrived:
//   k_spect_frame_stats  : per frame the fp64 sum and sum of squares of its 161 values, in an order that depends on the bin alone
//   k_spect_scan         : per clip (or stream) a STRICT left fold of those partials in frame order -- fp64 addition is not
//                          associative, and only the strict fold gives the same bits however the audio is cut into feeds --
//                          then mean_t / rstd_t per frame with k_spect_finalize's arithmetic
//   k_spect_write<., true> : the write kernel with per-frame statistics
// The streaming form (ds2_spect_stream_feed) runs the same kernels on a window [carried samples | new samples] per stream:
//   k_spect_stream_window / k_spect_stream_carry : assemble the windows in the workspace, then keep the samples that frames not
//                          yet complete will need (at most 319 a stream)
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
// GEMM: pt comes from the front-end's GEMM output (normalised as the write kernel normalises; fms [N][ld][2] = the per-frame
// statistics of the running normalisation); else from a batch (N, 1, F, ld).
// Zero coefficients (= no warp): null draw, i < 0 or i >= T, T <= 2W (the reference's randrange raises there), non-finite result.
template <bool GEMM>
__global__ void k_spect_warp_coef(const float* __restrict__ src, long strideN, int ld, const int* __restrict__ len,
                                  const float* __restrict__ ms, int normalize, const float* __restrict__ draw, int N, int F, int W,
                                  float* __restrict__ coef, float* __restrict__ coef_out, const float* __restrict__ fms = nullptr) {
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
      float mean = normalize ? ms[2 * n] : 0.f, rstd = normalize ? ms[2 * n + 1] : 1.f;
      if (fms) mean = fms[2 * ((long)n * ld + i)], rstd = fms[2 * ((long)n * ld + i) + 1];     // running: frame i's own statistics
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

// One row of a streaming feed (ds2_spect_stream_row of include/ds2hip.h)
struct SpectRow {
  int slot, src, carried, n_new, frames_before, emit, final_, fresh;
};

// grid (ceil(Tmax/64), 3, N): 64 frames x 64 bins per block through LDS; out[n][0][f][t].  AUG: every output takes its value
// from the clip's own frames fl, fl + 1 <= T - 1 (rows of the GEMM output are [t][LDC]: a wave reads 64 neighbouring bins of one
// or two rows, the transpose tile keeps the stores coalesced) and masked cells are written as 0.  RUN: every frame has its own
// mean / rstd, fms [N][Tmax][2] (null = none: raw log-magnitudes), and with `rows` the frame count of clip n is rows[n].emit.
template <bool AUG, bool RUN>
__global__ void __launch_bounds__(256) k_spect_write(const float* __restrict__ C, long strideC, const int* __restrict__ nsamp,
                                                     const float* __restrict__ ms, int normalize, float* __restrict__ out, int Tmax,
                                                     AugArgs aug, const float* __restrict__ fms, const SpectRow* __restrict__ rows) {
  __shared__ float tile[64][65];
  const int n = blockIdx.z, t0 = blockIdx.x * 64, f0 = blockIdx.y * 64;
  int T;
  if constexpr (RUN) T = rows ? min(max(rows[n].emit, 0), Tmax) : 1 + nsamp[n] / HOP;
  else T = 1 + nsamp[n] / HOP;
  float mean = 0.f, rstd = 1.f;
  if constexpr (!RUN) mean = normalize ? ms[2 * n] : 0.f, rstd = normalize ? ms[2 * n + 1] : 1.f;
  const float* Cn = C + (long)n * strideC;
  const float* fn = RUN && fms ? fms + (long)n * Tmax * 2 : nullptr;
  // the value of frame t, bin f as the model sees it
  auto value = [&](int t, int f) {
    if constexpr (RUN) {
      if (fn) return (logmag(Cn + (long)t * LDC, f) - fn[2 * t]) * fn[2 * t + 1];
      return logmag(Cn + (long)t * LDC, f);
    } else {
      return (logmag(Cn + (long)t * LDC, f) - mean) * rstd;
    }
  };
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
          const float lo = value(fl, f), hi = value(fl + 1, f);
          v = aug_lerp(lo, hi, alpha);
        } else {
          v = value(t, f);
        }
      } else {
        v = value(t, f);
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

// ---- running normalisation -----------------------------------------------------------------------------------------------
// grid (ceil(Tld/4), N), one wave per frame: sq[n][t] = (sum, sum of squares) of the frame's 161 values in fp64.  Lane l adds
// bins l, l + 64, l + 128 in that order, then the lanes are folded by a butterfly: the order depends on the bin alone, so a
// frame's partials are the same bits wherever the frame sits in a launch.
__global__ void __launch_bounds__(256) k_spect_frame_stats(const float* __restrict__ C, long strideC, const int* __restrict__ nsamp,
                                                           const SpectRow* __restrict__ rows, int Tld, double* __restrict__ sq) {
  const int n = blockIdx.y, t = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int T = rows ? min(max(rows[n].emit, 0), Tld) : min(1 + nsamp[n] / HOP, Tld);
  if (t >= T) return;                                            // wave-uniform
  const float* row = C + (long)n * strideC + (long)t * LDC;
  double s = 0.0, q = 0.0;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int f = lane + 64 * k;
    if (f < NBIN) {
      const double v = (double)logmag(row, f);
      s += v;
      q += v * v;
    }
  }
  for (int o = 32; o > 0; o >>= 1) {
    s += __shfl_xor(s, o, 64);
    q += __shfl_xor(q, o, 64);
  }
  if (lane == 0) {
    sq[2 * ((long)n * Tld + t)] = s;
    sq[2 * ((long)n * Tld + t) + 1] = q;
  }
}

struct RunArgs {            // the mode's two parameters, evaluated on the host in fp64
  double floor_;            // rstd = 1 / max(std, floor)
  double S0, Q0, cnt0;      // the prior's pseudo-counts: the state of a stream that has seen nothing (all 0 = none)
};

// grid (N), one workgroup per clip / stream: S_t = S_(t-1) + s[t], Q_t = Q_(t-1) + q[t] strictly in frame order.  256 frames'
// partials are staged in LDS at a time, thread 0 folds them (two dependent fp64 adds a frame, the LDS reads are off the chain),
// then every thread turns one frame's (S_t, Q_t) into mean_t / rstd_t with k_spect_finalize's arithmetic.  rows == null: clip n
// has 1 + nsamp[n] / 160 frames and starts from the prior; else row n starts from state[slot] (from the prior when the slot is
// fresh), its frames count on from frames_before, and state[slot] is written back.
__global__ void __launch_bounds__(256) k_spect_scan(const double* __restrict__ sq, const int* __restrict__ nsamp,
                                                    const SpectRow* __restrict__ rows, int Tld, RunArgs ra, double* __restrict__ state,
                                                    float* __restrict__ fms) {
  __shared__ double ls[256], lq[256];
  const int n = blockIdx.x, tid = threadIdx.x;
  int T, tb = 0;
  double* stp = nullptr;
  double S = ra.S0, Q = ra.Q0;
  if (rows) {
    const SpectRow R = rows[n];
    T = min(max(R.emit, 0), Tld);
    tb = R.frames_before;
    stp = state + 2 * (long)R.slot;
    if (!R.fresh) S = stp[0], Q = stp[1];
  } else {
    T = min(1 + nsamp[n] / HOP, Tld);
  }
  const double* sn = sq + 2 * (long)n * Tld;
  for (int c0 = 0; c0 < T; c0 += 256) {
    const int t = c0 + tid;
    if (t < T) {
      ls[tid] = sn[2 * t];
      lq[tid] = sn[2 * t + 1];
    }
    __syncthreads();
    if (tid == 0) {
      const int m = min(256, T - c0);
      for (int i = 0; i < m; ++i) {
        S += ls[i];
        Q += lq[i];
        ls[i] = S;
        lq[i] = Q;
      }
    }
    __syncthreads();
    if (t < T) {
      const double cnt = (double)NBIN * (double)(tb + t + 1) + ra.cnt0;
      const double mean = ls[tid] / cnt;
      double var = (lq[tid] - cnt * mean * mean) / (cnt - 1.0);
      if (var < 0.0) var = 0.0;
      const double sd = sqrt(var);
      fms[2 * ((long)n * Tld + t)] = (float)mean;
      fms[2 * ((long)n * Tld + t) + 1] = (float)(1.0 / (sd > ra.floor_ ? sd : ra.floor_));
    }
    __syncthreads();
  }
  if (tid == 0 && stp) {
    stp[0] = S;
    stp[1] = Q;
  }
}

// ---- streaming windows ---------------------------------------------------------------------------------------------------
constexpr int CARRY_LD = 320;      // floats a slot's carry occupies (at most 319 are used)

// grid (ceil(lw/256), n_rows): win[r] = [160 zeros if fresh | carry[slot][0:carried] | wav[src][0:n_new] | zeros to lw]; the
// zeros behind the new samples are the right centre padding of a final row and keep every GEMM row's reads defined.
__global__ void __launch_bounds__(256) k_spect_stream_window(const float* __restrict__ wav, long ldw, const SpectRow* __restrict__ rows,
                                                             const float* __restrict__ carry, float* __restrict__ win, long lw) {
  const int r = blockIdx.y;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= lw) return;
  const SpectRow R = rows[r];
  const int lead = R.fresh ? NFFT / 2 : 0, c = R.fresh ? 0 : min(max(R.carried, 0), CARRY_LD - 1);
  const long j = i - lead;
  float v = 0.f;
  if (j >= 0 && j < c) v = carry[(long)R.slot * CARRY_LD + j];
  else if (j >= c && j < (long)c + R.n_new) v = wav[(long)R.src * ldw + (j - c)];
  win[(long)r * lw + i] = v;
}

// grid (n_rows), 320 threads: the new carry = the window from the first frame that is not yet complete on, 160 emit <= i <
// the window's length (160 + (samples % 160) <= 319 values).  A separate launch: the carry words are read by the launch before.
__global__ void __launch_bounds__(CARRY_LD) k_spect_stream_carry(const SpectRow* __restrict__ rows, const float* __restrict__ win, long lw,
                                                                 float* __restrict__ carry) {
  const SpectRow R = rows[blockIdx.x];
  const int lead = R.fresh ? NFFT / 2 : 0, c = R.fresh ? 0 : min(max(R.carried, 0), CARRY_LD - 1);
  const long wl = (long)lead + c + R.n_new, from = (long)HOP * max(R.emit, 0) + threadIdx.x;
  if (R.final_ || from >= wl || from >= lw) return;             // a stream that has ended needs no carry
  carry[(long)R.slot * CARRY_LD + threadIdx.x] = win[(long)blockIdx.x * lw + from];
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
                     hipStream_t st, const RunArgs* run = nullptr) {
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
  float* fms = nullptr;
  if (run) {   // running normalisation: per-frame partials, the strict fold, per-frame mean / rstd behind the one-shot layout
    double* sq = (double*)(coef + 4L * N);
    fms = (float*)(sq + 2L * N * Tmax);
    hipLaunchKernelGGL(k_spect_frame_stats, dim3(ds2_cdiv(Tmax, 4), N), dim3(256), 0, st, (const float*)Cbuf, (long)Tmax * LDC, nsamples,
                       (const SpectRow*)nullptr, Tmax, sq);
    DS2_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_spect_scan, dim3(N), dim3(256), 0, st, (const double*)sq, nsamples, (const SpectRow*)nullptr, Tmax, *run,
                       (double*)nullptr, fms);
    DS2_CHECK_LAUNCH();
  } else if (normalize) {
    hipLaunchKernelGGL(k_spect_stats, dim3(STAT_BLOCKS, N), dim3(256), 0, st, (const float*)Cbuf, (long)Tmax * LDC, nsamples, partial);
    DS2_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_spect_finalize, dim3(ds2_cdiv(N, 64)), dim3(64), 0, st, (const double*)partial, nsamples, N, ms);
    DS2_CHECK_LAUNCH();
  }
  const dim3 grid(ds2_cdiv(Tmax, 64), 3, N);
  const float* Cc = Cbuf;
  const long sC = (long)Tmax * LDC;
  if (!aug) {
    if (run)
      hipLaunchKernelGGL((k_spect_write<false, true>), grid, dim3(256), 0, st, Cc, sC, nsamples, (const float*)ms, 0, out, Tmax, AugArgs{},
                         (const float*)fms, (const SpectRow*)nullptr);
    else
      hipLaunchKernelGGL((k_spect_write<false, false>), grid, dim3(256), 0, st, Cc, sC, nsamples, (const float*)ms, normalize, out, Tmax,
                         AugArgs{}, (const float*)nullptr, (const SpectRow*)nullptr);
    DS2_CHECK_LAUNCH();
    return 0;
  }
  hipLaunchKernelGGL(k_spect_warp_coef<true>, dim3(ds2_cdiv(N, 64)), dim3(64), 0, st, Cc, sC, Tmax, nsamples, (const float*)ms,
                     run ? 0 : normalize, warp_draw, N, NBIN, W, coef, coef_out, (const float*)fms);
  DS2_CHECK_LAUNCH();
  AugArgs a = *aug;
  a.coef = coef;
  if (run)
    hipLaunchKernelGGL((k_spect_write<true, true>), grid, dim3(256), 0, st, Cc, sC, nsamples, (const float*)ms, 0, out, Tmax, a,
                       (const float*)fms, (const SpectRow*)nullptr);
  else
    hipLaunchKernelGGL((k_spect_write<true, false>), grid, dim3(256), 0, st, Cc, sC, nsamples, (const float*)ms, normalize, out, Tmax, a,
                       (const float*)nullptr, (const SpectRow*)nullptr);
  DS2_CHECK_LAUNCH();
  return 0;
}

// floor and the prior (mean, std, frames; frames = 0: none) -> the scan's arguments, in fp64 on the host: one place for the one-shot
// and the streaming call, so both start from the same bits
bool run_args(double floor_, double pm, double ps, double pf, RunArgs& ra) {
  if (!(floor_ > 0.0) || !(pf >= 0.0) || !(ps >= 0.0) || !(pm == pm) || !(pf < 1e9)) return false;
  const double c = (double)NBIN * pf;
  ra = RunArgs{floor_, pm * c, (ps * ps + pm * pm) * c, c};
  return true;
}

inline long stream_win_len(int max_new) { return (((long)max_new + 2 * NFFT + 3) / 4) * 4 + NFFT; }

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

// ---- running (causal) normalisation: normalize = 2 -------------------------------------------------------------------------
// ds2_spect_ws_bytes + the per-frame partials [N][Tmax][2] f64 and statistics [N][Tmax][2] f32
long ds2_spect_running_ws_bytes(int N, int Lmax) {
  const long Tmax = 1 + Lmax / HOP;
  return ds2_spect_ws_bytes(N, Lmax) + (long)N * Tmax * (2 * 8 + 2 * 4);
}

// ds2_spectrogram / ds2_spectrogram_aug (aug != 0: with warp_draw .. coef_out as there) with frame t normalised by the mean and
// unbiased standard deviation of frames 0..t of its clip: rstd_t = 1 / max(std_t, floor).  prior_frames > 0: the statistics
// start from prior_frames pseudo-frames of mean prior_mean and standard deviation prior_std.
int ds2_spectrogram_running(const float* wav, long ldw, const int* nsamples, int N, int Lmax, const float* basis, int reflect,
                            double floor_, double prior_mean, double prior_std, double prior_frames, float* out, void* ws, int aug,
                            const float* warp_draw, int W, const int* fmask, int MF, const int* tmask, int MT, float* coef_out,
                            ds2_stream_t st_) {
  DS2_REQUIRE(wav && nsamples && basis && out && ws && N > 0 && N <= 65535 && Lmax > 0 && ldw >= Lmax, DS2_ERR_ARG);
  RunArgs ra;
  DS2_REQUIRE(run_args(floor_, prior_mean, prior_std, prior_frames, ra), DS2_ERR_ARG);
  if (!aug)
    return spectrogram_impl(wav, ldw, nsamples, N, Lmax, basis, reflect, 2, out, ws, nullptr, 0, nullptr, nullptr, (hipStream_t)st_, &ra);
  DS2_REQUIRE(W >= 0 && MF >= 0 && MF <= MAX_MASKS && MT >= 0 && MT <= MAX_MASKS && (fmask || MF == 0) && (tmask || MT == 0), DS2_ERR_ARG);
  const AugArgs a{nullptr, fmask, tmask, MF, MT};
  return spectrogram_impl(wav, ldw, nsamples, N, Lmax, basis, reflect, 2, out, ws, warp_draw, W, &a, coef_out, (hipStream_t)st_, &ra);
}

// ---- the streaming front-end -------------------------------------------------------------------------------------------------
// Host only.  After samples_before samples of a stream, a feed of n_new more (final != 0: the last of the utterance):
//   out[0] frames complete before the feed (samples_before / 160), out[1] frames the feed emits, out[2] samples the window takes
//   from the carry (160 + samples_before % 160, the left centre padding included), out[3] the window's length (with the 160 zeros
//   of a final feed), out[4] the samples carried on (0 after a final feed), out[5] the position of the window's first sample in
//   the clip (-160 while the window starts inside the left padding).
int ds2_spect_stream_plan(long samples_before, int n_new, int final_, int* out) {
  DS2_REQUIRE(out != nullptr && samples_before >= 0 && n_new >= 0 && samples_before + n_new < (1L << 30), DS2_ERR_ARG);
  const long f0 = samples_before / HOP, g1 = samples_before + n_new;
  const long f1 = final_ ? 1 + g1 / HOP : g1 / HOP;
  const long carried = HOP + samples_before % HOP, wl = carried + n_new + (final_ ? HOP : 0);
  out[0] = (int)f0;
  out[1] = (int)(f1 - f0);
  out[2] = (int)carried;
  out[3] = (int)wl;
  out[4] = final_ ? 0 : (int)(wl - HOP * (f1 - f0));
  out[5] = (int)(HOP * f0 - HOP);
  return 0;
}

// per slot: the running sums (S, Q) f64, then [S][320] f32 carried samples
long ds2_spect_stream_state_bytes(int S) { return S > 0 ? (long)S * (2 * 8 + CARRY_LD * 4) : 0; }
// windows [n_rows][lw] + GEMM output [n_rows][Tc][336] + per-frame statistics f32, then the per-frame partials f64
long ds2_spect_stream_ws_bytes(int n_rows, int max_new, int Tc) {
  if (n_rows <= 0 || max_new < 0 || Tc < 0) return -1;
  return (((long)n_rows * stream_win_len(max_new) + (long)n_rows * Tc * LDC + 2L * n_rows * Tc) * 4 + 15) / 16 * 16 + 2L * n_rows * Tc * 8;
}

// One feed of n_rows streams.  wav [.][ldw] f32: row r's n_new new samples are wav[rows[r].src][0 : n_new], n_new <= max_new <=
// ldw (null for max_new = 0).  rows [n_rows] ds2_spect_stream_row on the device, as ds2_spect_stream_plan gives them: `carried`
// = out[2] (0 for a fresh slot, whose carry reads as the 160 zeros of the left padding and whose statistics start from the
// prior), frames_before = out[0], emit = out[1] <= Tc.  normalize: 0 raw log-magnitudes, 2 running; 1 is refused (not causal).
// state: ds2_spect_stream_state_bytes(S) bytes, 8-byte aligned; slots that are not in `rows` are not touched.  out (n_rows, 1,
// 161, Tc) f32 in table order, frames >= the row's emit are zero; Tc = 0 only moves the carries.  The table lives on the device:
// slots must be distinct and lie in [0, S), and the counts must be the plan's (spectrogram.SpectStream checks them on the host).
int ds2_spect_stream_feed(const float* wav, long ldw, const ds2_spect_stream_row* rows, int n_rows, int max_new, int Tc, int S,
                          const float* basis, int normalize, double floor_, double prior_mean, double prior_std, double prior_frames,
                          void* state, float* out, void* ws, ds2_stream_t st_) {
  hipStream_t st = (hipStream_t)st_;
  static_assert(sizeof(ds2_spect_stream_row) == sizeof(SpectRow), "row table layout");
  DS2_REQUIRE(rows && basis && state && ws && n_rows > 0 && n_rows <= 65535 && S >= n_rows && max_new >= 0 && Tc >= 0, DS2_ERR_ARG);
  DS2_REQUIRE((wav && ldw >= max_new) || max_new == 0, DS2_ERR_ARG);
  DS2_REQUIRE((out || Tc == 0) && (normalize == 0 || normalize == 2), DS2_ERR_ARG);
  const long lw = stream_win_len(max_new);
  DS2_REQUIRE((long)HOP * Tc + HOP <= lw, DS2_ERR_ARG);          // every GEMM row reads inside its window
  RunArgs ra;
  DS2_REQUIRE(run_args(floor_, prior_mean, prior_std, prior_frames, ra), DS2_ERR_ARG);
  const SpectRow* R = (const SpectRow*)rows;
  double* sums = (double*)state;
  float* carry = (float*)(sums + 2L * S);
  float* win = (float*)ws;
  float* Cbuf = win + (long)n_rows * lw;
  float* fms = Cbuf + (long)n_rows * Tc * LDC;
  double* sq = (double*)(((uintptr_t)(fms + 2L * n_rows * Tc) + 15) & ~(uintptr_t)15);
  hipLaunchKernelGGL(k_spect_stream_window, dim3(ds2_cdiv(lw, 256), n_rows), dim3(256), 0, st, wav, ldw, R, (const float*)carry, win, lw);
  DS2_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_spect_stream_carry, dim3(n_rows), dim3(CARRY_LD), 0, st, R, (const float*)win, lw, carry);
  DS2_CHECK_LAUNCH();
  if (Tc > 0) {
    int rc = ds2_gemm_nt(DS2_F32, win, basis, Cbuf, nullptr, Tc, 2 * NBIN, NFFT, HOP, NFFT, LDC, 1, n_rows, lw, 0, (long)Tc * LDC, 0, 1,
                         (ds2_stream_t)st);
    if (rc != 0) return rc;
  }
  if (normalize == 2) {
    if (Tc > 0) {
      hipLaunchKernelGGL(k_spect_frame_stats, dim3(ds2_cdiv(Tc, 4), n_rows), dim3(256), 0, st, (const float*)Cbuf, (long)Tc * LDC,
                         (const int*)nullptr, R, Tc, sq);
      DS2_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(k_spect_scan, dim3(n_rows), dim3(256), 0, st, (const double*)sq, (const int*)nullptr, R, Tc, ra, sums, fms);
    DS2_CHECK_LAUNCH();
  }
  if (Tc > 0) {
    hipLaunchKernelGGL((k_spect_write<false, true>), dim3(ds2_cdiv(Tc, 64), 3, n_rows), dim3(256), 0, st, (const float*)Cbuf, (long)Tc * LDC,
                       (const int*)nullptr, (const float*)nullptr, 0, out, Tc, AugArgs{}, normalize == 2 ? (const float*)fms : nullptr, R);
    DS2_CHECK_LAUNCH();
  }
  return 0;
}

}  // extern "C"
