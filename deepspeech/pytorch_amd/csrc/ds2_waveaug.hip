// Waveform augmentation on the device: what SpectrogramParser.parse_audio does to the samples BEFORE the STFT (reference
// loader/data_loader.py:151-159): load_randomly_augmented_audio (:377-404, sox `tempo t gain g`) and NoiseInjection.inject_noise
// (:97-128).  All kernels work on the [N][ld] fp32 waveform batch that ds2_spectrogram takes, with per-clip sample counts on the
// device, write out of place, and write every entry beyond a clip's own samples as zero (the spectrogram's centre padding reads
// them).
//   k_wsola       : tempo change at constant pitch by waveform-similarity overlap-add, one workgroup per clip (the segments of a
//                   clip depend on each other through the chosen offset; clips are independent)
//   k_wave_energy : per clip the sum of squares of the gained, clamped data and of its noise crop; EBLOCKS workgroups per clip,
//                   fp64, fixed-order partials (no atomics: the sums are the same bits from launch to launch)
//   k_wave_mix    : out = clamp(g x) + scale * noise, scale = level * sqrt(E_data / E_noise) from the partials
// The energy / mix pair stays two launches: a kernel boundary costs ~1.5 us, any grid-wide step inside one launch costs more.
//
// WSOLA (DESIGN.md section 7 has the rules in full).  Parameters = sox `tempo` defaults at 16 kHz: segment 1312 samples (82 ms),
// 234 candidate offsets (14.68 ms), overlap 192 samples (12 ms); a segment advances the output by ADV = 1312 - 192 = 1120 samples.
//   start(k) = floor(k * tempo * 1120)                                         (fp64, tempo widened from fp32)
//   S        = number of k with start(k) + 192 <= L                            (every segment can complete its cross-fade)
//   out_len  = (S - 1) * 1120 + min(1312, L - start(S - 1))                    (the last segment is flushed to the clip's end)
//   p(0) = 0;  p(k) = start(k) + d(k),  d(k) = the lowest arg-max over d in [0, 234) of  sum_j x[p(k-1) + 1120 + j] * x[start(k) + d + j],
//   j in [0, 192): the previous segment's tail against the input; reads at or beyond L are zero
//   out[1120 k + j] = x[p(k) + j], and for k >= 1, j < 192:  a + (j / 192) * (x[p(k) + j] - a),  a = x[p(k-1) + 1120 + j]
// A clip with L < 1312 + 234, or a tempo outside [0.1, 10] (NaN included), is copied unchanged.
// The dot product is fp32: four partial sums over j = c (mod 4), fused multiply-adds in rising j, combined as (s0 + s1) + (s2 + s3).
#include "ds2_common.h"

namespace {

constexpr int SEG = 1312, SEARCH = 234, OVL = 192, ADV = SEG - OVL;
constexpr int WIN = SEARCH + OVL;        // samples of the input a segment's search reads (d + j <= 233 + 191)
constexpr int EBLOCKS = 8;               // workgroups per clip of the energy kernel
constexpr int ESTRIDE = EBLOCKS * 256;   // samples one sweep of a clip's workgroups covers

__host__ __device__ inline bool wsola_runs(long L, float tempo) { return L >= SEG + SEARCH && tempo >= 0.1f && tempo <= 10.f; }
__host__ __device__ inline long wsola_start(long k, float tempo) { return (long)floor((double)k * (double)tempo * (double)ADV); }
__host__ __device__ inline long wsola_segments(long L, float tempo) {
  if (!wsola_runs(L, tempo)) return 0;
  long k = (long)((double)(L - OVL) / ((double)tempo * (double)ADV));      // an estimate; the two loops make it exact
  while (wsola_start(k + 1, tempo) + OVL <= L) ++k;
  while (k > 0 && wsola_start(k, tempo) + OVL > L) --k;
  return k + 1;
}
__host__ __device__ inline long wsola_out_len(long L, float tempo) {
  const long S = wsola_segments(L, tempo);
  if (S == 0) return L < 0 ? 0 : L;
  const long rem = L - wsola_start(S - 1, tempo);
  return (S - 1) * ADV + (rem < SEG ? rem : SEG);
}

// grid (N), 256 threads.  LDS: the search window of the current segment, the previous segment's tail, the four wave maxima.
__global__ void __launch_bounds__(256) k_wsola(const float* __restrict__ x, long ldx, const int* __restrict__ nsamp,
                                               const float* __restrict__ tempo, float* __restrict__ out, long ldo,
                                               int* __restrict__ nsamp_out, int* __restrict__ offsets, int Smax) {
  __shared__ __attribute__((aligned(16))) float tail[OVL];
  __shared__ float win[WIN + 2];
  __shared__ float redv[4];
  __shared__ int redd[4];
  const int n = blockIdx.x, tid = threadIdx.x;
  const float* xn = x + (long)n * ldx;
  float* on = out + (long)n * ldo;
  long L = nsamp[n];
  L = L < 0 ? 0 : (L > ldx ? ldx : L);
  const float tp = tempo ? tempo[n] : 0.f;                 // no tempo array: every clip is copied
  const long S = wsola_segments(L, tp);
  const long olen = wsola_out_len(L, tp);
  if (tid == 0) nsamp_out[n] = (int)(olen < ldo ? olen : ldo);
  for (long k = tid; k < Smax; k += 256)
    if (k >= S) offsets[(long)n * Smax + k] = -1;
  if (S == 0) {
    for (long i = tid; i < ldo; i += 256) on[i] = i < L ? xn[i] : 0.f;
    return;
  }
  long prev = 0;                                           // p(k - 1)
  for (long k = 0; k < S; ++k) {
    const long st = wsola_start(k, tp);
    int d = 0;
    if (k > 0) {                                           // win = x[st ..], tail = x[prev + ADV ..] were staged by the previous turn
      float v = -INFINITY;
      int dd = 0;
      if (tid < SEARCH) {
        float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
        const float* w = win + tid;
#pragma unroll 8
        for (int j = 0; j < OVL; j += 4) {
          const float4 t = *reinterpret_cast<const float4*>(tail + j);      // one broadcast read
          s0 = fmaf(t.x, w[j], s0);
          s1 = fmaf(t.y, w[j + 1], s1);
          s2 = fmaf(t.z, w[j + 2], s2);
          s3 = fmaf(t.w, w[j + 3], s3);
        }
        v = (s0 + s1) + (s2 + s3);
        dd = tid;
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {                   // arg-max, the lowest offset among equal values
        const float ov = __shfl_xor(v, o, 64);
        const int od = __shfl_xor(dd, o, 64);
        if (ov > v || (ov == v && od < dd)) v = ov, dd = od;
      }
      if ((tid & 63) == 0) redv[tid >> 6] = v, redd[tid >> 6] = dd;
      __syncthreads();
      v = redv[0], dd = redd[0];
#pragma unroll
      for (int w = 1; w < 4; ++w)
        if (redv[w] > v || (redv[w] == v && redd[w] < dd)) v = redv[w], dd = redd[w];
      d = dd < 0 ? 0 : (dd >= SEARCH ? SEARCH - 1 : dd);   // in range whatever the samples hold (NaN compares false everywhere)
    }
    if (tid == 0 && k < Smax) offsets[(long)n * Smax + k] = d;
    const long p = st + d;
    // the next turn's window and tail, into registers now so that their latency overlaps this turn's copy
    float r0 = 0.f, r1 = 0.f, rt = 0.f;
    const bool more = k + 1 < S;
    if (more) {
      const long s1 = wsola_start(k + 1, tp);
      if (s1 + tid < L) r0 = xn[s1 + tid];
      if (tid + 256 < WIN && s1 + 256 + tid < L) r1 = xn[s1 + 256 + tid];
      if (tid < OVL && p + ADV + tid < L) rt = xn[p + ADV + tid];
    }
    const long o0 = k * ADV;
    const int len = more ? ADV : (int)(L - st < SEG ? L - st : SEG);
    for (int j = tid; j < len; j += 256) {
      float b = p + j < L ? xn[p + j] : 0.f;
      if (k > 0 && j < OVL) {
        const float a = tail[j];
        b = fmaf((float)j / (float)OVL, b - a, a);
      }
      if (o0 + j < ldo) on[o0 + j] = b;
    }
    prev = p;
    __syncthreads();                                       // every read of win / tail / red of this turn is done
    if (more) {
      win[tid] = r0;
      if (tid + 256 < WIN) win[tid + 256] = r1;
      if (tid < OVL) tail[tid] = rt;
    }
    __syncthreads();
  }
  for (long i = olen + tid; i < ldo; i += 256) on[i] = 0.f;
}

struct NoiseArgs {
  const float* level;            // [N], null = no noise at all; <= 0 = none for the clip
  const float* bank;             // the noise recordings back to back
  long bank_len;
  const long long* off;          // [N] first sample of the clip's recording in the bank, negative = none for the clip
  const int* start;              // [N] first sample of the crop inside the recording
};

__device__ __forceinline__ float gained(const float* __restrict__ gain, int n, float v) {
  return gain ? fminf(fmaxf(gain[n] * v, -1.f), 1.f) : v;
}
__device__ __forceinline__ bool has_noise(const NoiseArgs& a, int n) { return a.level && a.level[n] > 0.f && a.off[n] >= 0; }
__device__ __forceinline__ float noise_at(const NoiseArgs& a, long base, long i) {
  const long idx = base + i;
  return idx >= 0 && idx < a.bank_len ? a.bank[idx] : 0.f;
}

// grid (EBLOCKS, N): thread t of block b takes samples b * 256 + t + m * ESTRIDE.  partial [N][EBLOCKS][2] f64.
__global__ void __launch_bounds__(256) k_wave_energy(const float* __restrict__ x, long ldx, const int* __restrict__ nsamp,
                                                     const float* __restrict__ gain, NoiseArgs na, double* __restrict__ partial) {
  __shared__ double red[2][4];
  const int n = blockIdx.y;
  long L = nsamp[n];
  L = L < 0 ? 0 : (L > ldx ? ldx : L);
  const float* xn = x + (long)n * ldx;
  const bool noisy = has_noise(na, n);
  const long base = noisy ? (long)na.off[n] + na.start[n] : 0;
  double s = 0.0, q = 0.0;
  for (long i = blockIdx.x * 256 + threadIdx.x; i < L; i += ESTRIDE) {
    const double y = (double)gained(gain, n, xn[i]);
    s += y * y;
    if (noisy) {
      const double v = (double)noise_at(na, base, i);
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
    partial[((long)n * EBLOCKS + blockIdx.x) * 2] = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
    partial[((long)n * EBLOCKS + blockIdx.x) * 2 + 1] = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
  }
}

// grid (ceil(ldo / 1024), N): four samples per thread, 256 apart.  The noise term is one fused multiply-add in fp32.
__global__ void __launch_bounds__(256) k_wave_mix(const float* __restrict__ x, long ldx, const int* __restrict__ nsamp,
                                                  const float* __restrict__ gain, NoiseArgs na, const double* __restrict__ partial,
                                                  float* __restrict__ out, long ldo) {
  __shared__ float scale_s;
  const int n = blockIdx.y;
  long L = nsamp[n];
  L = L < 0 ? 0 : (L > ldx ? ldx : L);
  const bool noisy = has_noise(na, n);
  if (threadIdx.x == 0) {
    float sc = 0.f;
    if (noisy) {
      double ed = 0.0, en = 0.0;
      for (int b = 0; b < EBLOCKS; ++b) {
        ed += partial[((long)n * EBLOCKS + b) * 2];
        en += partial[((long)n * EBLOCKS + b) * 2 + 1];
      }
      if (en > 0.0) sc = (float)((double)na.level[n] * sqrt(ed / en));    // a silent crop adds nothing (the reference: NaN)
    }
    scale_s = sc;
  }
  __syncthreads();
  const float sc = scale_s;
  const long base = noisy ? (long)na.off[n] + na.start[n] : 0;
  const float* xn = x + (long)n * ldx;
  float* on = out + (long)n * ldo;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const long i = (long)blockIdx.x * 1024 + r * 256 + threadIdx.x;
    if (i >= ldo) break;
    float v = 0.f;
    if (i < L) {
      v = gained(gain, n, xn[i]);
      if (sc != 0.f) v = fmaf(sc, noise_at(na, base, i), v);
    }
    on[i] = v;
  }
}

}  // namespace

extern "C" {

// segments and output samples of a clip of `nsamples` samples at `tempo` (host-only queries; 0 segments = the clip is copied)
int ds2_wsola_segments(int nsamples, float tempo) { return (int)wsola_segments(nsamples, tempo); }
long ds2_wsola_out_len(int nsamples, float tempo) { return wsola_out_len(nsamples, tempo); }

int ds2_wsola(const float* wav, long ldw, const int* nsamples, const float* tempo, int N, float* out, long ldo, int* nsamples_out,
              int* offsets, int Smax, ds2_stream_t st_) {
  hipStream_t st = (hipStream_t)st_;
  DS2_REQUIRE(wav && nsamples && out && nsamples_out && wav != out && N > 0 && ldw > 0 && ldo > 0 && ldo <= 0x7fffffffL, DS2_ERR_ARG);
  DS2_REQUIRE(Smax >= 0 && (offsets || Smax == 0), DS2_ERR_ARG);
  hipLaunchKernelGGL(k_wsola, dim3(N), dim3(256), 0, st, wav, ldw, nsamples, tempo, out, ldo, nsamples_out, offsets, Smax);
  DS2_CHECK_LAUNCH();
  return 0;
}

// bytes of the energy partials that ds2_wave_energy writes and ds2_wave_mix reads: [N][8][2] f64
long ds2_wave_ws_bytes(int N) { return (long)N * EBLOCKS * 2 * 8; }

int ds2_wave_energy(const float* wav, long ldw, const int* nsamples, int N, const float* gain, const float* level,
                    const float* bank, long bank_len, const long long* noise_off, const int* noise_start, void* ws,
                    ds2_stream_t st_) {
  hipStream_t st = (hipStream_t)st_;
  DS2_REQUIRE(wav && nsamples && ws && N > 0 && N <= 65535 && ldw > 0, DS2_ERR_ARG);
  DS2_REQUIRE(!level || (bank && bank_len > 0 && noise_off && noise_start), DS2_ERR_ARG);
  DS2_REQUIRE(((uintptr_t)ws & 7) == 0, DS2_ERR_ALIGN);
  hipLaunchKernelGGL(k_wave_energy, dim3(EBLOCKS, N), dim3(256), 0, st, wav, ldw, nsamples, gain,
                     NoiseArgs{level, bank, bank_len, noise_off, noise_start}, (double*)ws);
  DS2_CHECK_LAUNCH();
  return 0;
}

int ds2_wave_mix(const float* wav, long ldw, const int* nsamples, int N, const float* gain, const float* level, const float* bank,
                 long bank_len, const long long* noise_off, const int* noise_start, const void* ws, float* out, long ldo,
                 ds2_stream_t st_) {
  hipStream_t st = (hipStream_t)st_;
  DS2_REQUIRE(wav && nsamples && out && wav != out && N > 0 && N <= 65535 && ldw > 0 && ldo > 0, DS2_ERR_ARG);
  DS2_REQUIRE(!level || (bank && bank_len > 0 && noise_off && noise_start && ws), DS2_ERR_ARG);
  DS2_REQUIRE(((uintptr_t)ws & 7) == 0, DS2_ERR_ALIGN);
  hipLaunchKernelGGL(k_wave_mix, dim3(ds2_cdiv(ldo, 1024), N), dim3(256), 0, st, wav, ldw, nsamples, gain,
                     NoiseArgs{level, bank, bank_len, noise_off, noise_start}, (const double*)ws, out, ldo);
  DS2_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
