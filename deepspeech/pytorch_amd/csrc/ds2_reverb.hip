// Reverberation on the device: every clip of the [N][ld] fp32 waveform batch convolved with ITS room impulse response out of a
// device-resident bank (augment.RirBank), time-aligned on the response's direct-path tap (DESIGN.md section 7.1 "Reverberation").
// For clip n with L samples x, a response h of K taps and its peak index p:
//   out[i] = sum_{k = 0}^{K - 1} h[k] * x[i + p - k]   for 0 <= i < L,  x = 0 outside [0, L);   out[i] = 0 for L <= i < ldo
// A clip without a response (rir_off[n] < 0, or a null rir_off) is copied.  fp32 throughout, no clamp.
//
// k_reverb: a direct-form FIR as a block-Toeplitz product on v_mfma_f32_32x32x2_f32 (bitwise a chain of fp32 fused multiply-adds).
// With the shifted signal xs[m] = x[m + p] cut into blocks of 32, the 1024 outputs from a multiple `t` of 32 form the 32 x 32 matrix
// Y[i][b] = out[t + 32 b + i], and
//   Y = sum_q T_q X_q,   T_q[i][r] = h[32 q + i - r],   X_q[r][b] = xs[t + 32 (b - q) + r],   q = 0 .. (K + 30) / 32
// (h = 0 outside [0, K)).  One MFMA takes two values of r: lane l holds A = T_q[l & 31][2 s + (l >> 5)] and B = X_q[2 s + (l >> 5)][l & 31].
// Summation order of one output i: from +0, q rising, inside q r rising -- tap k = 32 q + (i mod 32) - r falls through a block of 32
// -- so it depends on i mod 32 and K alone; terms whose tap lies outside [0, K) enter as h = 0 (they add +0 * x).  No atomics, no
// split of a sum: one wave owns an output from the first term to the store.
// Work split: grid (ceil(ldo / TILE), N), 256 threads; wave w of a workgroup owns NACC matrices = NACC * 1024 consecutive outputs.
// The taps are walked in chunks of QC blocks (2048 taps): per chunk the workgroup stages the taps it touches and the clip window
// [tile - 32 (q0 + QC - 1), tile + TILE - 32 q0) in LDS, the window with a row pitch of 33 floats (the B read has a lane stride of 32
// samples; 33 spreads it over the banks).  A row loops over its own K only, a tile only over the blocks that reach samples at or
// after the clip's start, and a row without a response or a tile beyond the clip never gets to the MFMA loop.
#include "ds2_common.h"

namespace {

constexpr int NACC = 2;                            // 32 x 32 output matrices per wave
constexpr int TILE = 4 * NACC * 1024;              // consecutive outputs of one workgroup
constexpr int QC = 64;                             // blocks of 32 taps per chunk
constexpr int XBLOCKS = TILE / 32 + QC - 1;        // blocks of 32 samples in the staged window
constexpr int HS = 32 * QC + 64;                   // staged taps: h[32 q0 - 32 .. 32 (q0 + QC) + 32)

__global__ void __launch_bounds__(256) k_reverb(const float* __restrict__ x, long ldx, const int* __restrict__ nsamp,
                                                const float* __restrict__ bank, long bank_len, const long long* __restrict__ rir_off,
                                                const int* __restrict__ rir_len, const int* __restrict__ rir_peak,
                                                float* __restrict__ out, long ldo) {
  __shared__ float xs[XBLOCKS * 33];
  __shared__ float hs[HS];
  const int n = blockIdx.y, tid = threadIdx.x;
  const long tile = (long)blockIdx.x * TILE;
  const float* xn = x + (long)n * ldx;
  float* on = out + (long)n * ldo;
  long L = nsamp[n];
  L = L < 0 ? 0 : (L > ldx ? ldx : L);
  const long long off = rir_off ? rir_off[n] : -1;
  const long end = tile + TILE < ldo ? tile + TILE : ldo;
  if (off < 0 || tile >= L) {                      // the copy path, and the zeros beyond the clip
    for (long i = tile + tid; i < end; i += 256) on[i] = off < 0 && i < L ? xn[i] : 0.f;
    return;
  }
  const long K = rir_len[n] > 0 ? rir_len[n] : 0;
  const long p = rir_peak[n];
  long nq = K > 0 ? (K + 30) / 32 + 1 : 0;         // blocks q that hold a tap of [0, K)
  const long reach = (tile + TILE + p + 31) / 32 + 1;    // blocks q >= reach see samples in front of the clip only (p >= -tile)
  if (tile + TILE + p < 0) nq = 0;
  else if (nq > reach) nq = reach;

  const int lane = tid & 63, wave = tid >> 6, col = lane & 31, half = lane >> 5;
  ds2_f32x16 acc[NACC];
#pragma unroll
  for (int a = 0; a < NACC; ++a)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[a][r] = 0.f;

  for (long q0 = 0; q0 < nq; q0 += QC) {
    if (q0) __syncthreads();                       // the previous chunk's reads are done
    const long w0 = tile - 32 * (q0 + QC - 1) + p; // clip index of the window's first sample
    for (int u = tid; u < XBLOCKS * 32; u += 256) {
      const long xi = w0 + u;
      xs[u + (u >> 5)] = xi >= 0 && xi < L ? xn[xi] : 0.f;
    }
    const long h0 = 32 * q0 - 32;                  // tap index of hs[0]
    for (int v = tid; v < HS; v += 256) {
      const long k = h0 + v;
      const long long bi = off + k;
      hs[v] = k >= 0 && k < K && bi < bank_len ? bank[bi] : 0.f;
    }
    __syncthreads();
    const int qn = nq - q0 < QC ? (int)(nq - q0) : QC;
    // block (q0 + dq): A = hs[32 dq + 32 + col - r], B of matrix a = window block (wave * NACC + a) * 32 + col + QC - 1 - dq, entry r
    const float* ha = hs + 32 + col - half;
    const float* xb = xs + ((wave * NACC) * 32 + col + QC - 1) * 33 + half;
    for (int dq = 0; dq < qn; ++dq) {
#pragma unroll
      for (int s = 0; s < 16; ++s) {
        const float av = ha[32 * dq - 2 * s];
#pragma unroll
        for (int a = 0; a < NACC; ++a)
          acc[a] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, xb[(a * 32 - dq) * 33 + 2 * s], acc[a], 0, 0, 0);
      }
    }
  }
#pragma unroll
  for (int a = 0; a < NACC; ++a)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const long i = tile + (long)(wave * NACC + a) * 1024 + 32 * col + mma32_row(r, lane);
      if (i < end) on[i] = i < L ? acc[a][r] : 0.f;
    }
}

}  // namespace

extern "C" {

// consecutive outputs one workgroup computes (host-only query; the tests put clip lengths on its seams)
int ds2_reverb_tile(void) { return TILE; }

int ds2_reverb(const float* wav, long ldw, const int* nsamples, int N, const float* bank, long bank_len, const long long* rir_off,
               const int* rir_len, const int* rir_peak, float* out, long ldo, ds2_stream_t st_) {
  hipStream_t st = (hipStream_t)st_;
  DS2_REQUIRE(wav && nsamples && out && wav != out && N > 0 && N <= 65535 && ldw > 0 && ldo > 0, DS2_ERR_ARG);
  DS2_REQUIRE(!rir_off || (bank && rir_len && rir_peak), DS2_ERR_ARG);
  hipLaunchKernelGGL(k_reverb, dim3(ds2_cdiv(ldo, TILE), N), dim3(256), 0, st, wav, ldw, nsamples, bank, bank_len, rir_off, rir_len,
                     rir_peak, out, ldo);
  DS2_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
