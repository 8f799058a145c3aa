// Rational polyphase resampling to the front-end's 16 kHz on the device, one-shot and streamed (DESIGN.md section 7.2 has the
// definition in full; the reference converts its corpora with sox `rate` in offline scripts, this is the project's own filter).
//   g = gcd(in_rate, 16000), U = 16000 / g, D = in_rate / g, W = the half-width in input samples; a phase has 2W taps.
//   output m:  n0 = floor(m D / U), p = (m D) mod U (64-bit),  y[m] = sum_j h[p][j] x[n0 - W + 1 + j],  x = 0 outside the clip
//   out_len(n) = ceil(n U / D)
// The taps h [U][2W] f32 are the caller's (resample.Resampler builds them in fp64 on the host): the kernels only multiply and add.
// ORDER OF THE SUM: acc = 0, then acc = fma(h[p][j], x[.], acc) for j = 0 .. 2W - 1 in rising j, in every kernel and every path
// below.  It depends on the tap index alone -- not on where m falls in a tile, not on the launch, not on how a stream was cut into
// feeds -- so the streamed samples are the one-shot samples bit for bit.
//   k_resample        : grid (ceil(ldo / tile), N).  One workgroup = `tile` = P K consecutive outputs of one clip; their input
//                       span, at most (tile - 1) D / U + 1 + 2W samples, is staged in LDS once (zeros outside the clip).  P is a
//                       multiple of U, so the outputs i, i + P, i + 2P, ... of a tile share their phase: a thread takes K <= 16
//                       of them, loads its phase's taps eight at a time into registers and uses each for all K outputs.  Per
//                       product that leaves one LDS read (the sample); neighbouring lanes read neighbouring span entries.
//   k_resample_stream : the same tile body on the window [carry | new samples] of a stream; one more workgroup per row writes
//                       the samples the next feed needs into the workspace.
//   k_resample_stream_carry : workspace -> the slot's carry.  A launch of its own: the carry is read by the launch before.
// Where the taps live: in global memory, read through L1 / L2 into registers.  A thread walks ONE row of the table (its phase)
// per K outputs, so a table of 84 KiB (44100 Hz) or 120 KiB (11025 Hz) costs 2W / K loads per output and stays L2-resident; with
// U <= 2 (8, 32, 48 kHz) all lanes read the same one or two rows and the loads are L1 broadcasts.  The workgroup has 256 or 192
// threads, whichever leaves fewer lanes without a phase (U = 160: P = 160 on 192 threads).  A rate whose 2W + D / U samples do
// not fit the LDS span budget (multiples of 16 kHz beyond 592 kHz) reads the input from global memory instead; the sum is the same.
#include <algorithm>

#include "ds2_common.h"

namespace {

constexpr int RS_THREADS = 256;             // the largest workgroup
constexpr int RS_K = 16;                    // outputs of one phase a thread accumulates at most
constexpr long RS_SPAN_MAX = 11264;         // floats of LDS for the input span (44 KiB: three workgroups per CU)
constexpr long RS_TABLE_MAX = 131072;       // bytes of the largest table the entries accept

struct RsCfg {
  int nt;          // threads of a workgroup
  int P;           // outputs between two outputs of one thread: a multiple of U
  int K;           // outputs per thread
  int tile;        // P * K
  long cap;        // floats of the span (0 = the input is read from global memory)
  size_t lds;      // dynamic LDS bytes
};

inline bool rs_shape_ok(int U, int D, int W) { return U >= 1 && D >= 1 && W >= 1 && (long)U * 2 * W * 4 <= RS_TABLE_MAX; }

// floats of the span of P K consecutive outputs
inline long rs_cap(int P, int K, int U, int D, int W) { return (((long)P * K - 1) * D) / U + 1 + 2L * W; }

inline RsCfg rs_cfg(int U, int D, int W) {
  RsCfg c;
  double best = -1.0;
  for (int nt : {256, 192}) {
    const int P = U <= nt ? U * (nt / U) : U;
    const double eff = (double)P / ((double)((P + nt - 1) / nt) * nt);
    if (eff > best + 1e-9) best = eff, c.nt = nt, c.P = P;
  }
  c.K = 1, c.cap = 0;
  for (int k = RS_K; k >= 1; --k) {
    const long cap = rs_cap(c.P, k, U, D, W);
    if (cap <= RS_SPAN_MAX) {
      c.K = k, c.cap = cap;
      break;
    }
  }
  c.tile = c.P * c.K;
  c.lds = (size_t)c.cap * 4;
  return c;
}

__host__ __device__ inline long rs_cdiv(long a, long b) { return (a + b - 1) / b; }
// outputs that exist after G input samples: every one at the end of the utterance, else those whose last tap has arrived
__host__ __device__ inline long rs_outputs(long G, int final_, int U, int D, int W) {
  if (final_) return rs_cdiv(G * U, D);
  return G <= W ? 0 : rs_cdiv((G - W) * U, D);
}
// the first input sample that output m reads, clamped into the clip
__host__ __device__ inline long rs_first_input(long m, int U, int D, int W) {
  const long a = (m * D) / U - W + 1;
  return a < 0 ? 0 : a;
}

// a clip of n samples at x
struct ClipSrc {
  const float* x;
  long n;
  __device__ __forceinline__ float at(long i) const { return i >= 0 && i < n ? x[i] : 0.f; }
};
// the window of a stream: clip positions [first, first + carried) from the slot's carry, [first + carried, end) from the new samples
struct StreamSrc {
  const float* carry;
  const float* wav;
  long first, end;
  int carried;
  __device__ __forceinline__ float at(long i) const {
    if (i < first || i >= end) return 0.f;
    const long k = i - first;
    return k < carried ? carry[k] : wav[k - carried];
  }
};

// One row of a streaming feed (ds2_resample_stream_row of include/ds2hip.h)
struct ResampleRow {
  int slot, src, carried, n_new;
  long long out_before;
  int emit, final_, fresh, pad;
};

__device__ __forceinline__ StreamSrc stream_src(const ResampleRow& R, const float* carry, const float* wav, long ldw, int max_new, int U, int D,
                                                int W) {
  StreamSrc s;
  const int c = R.fresh ? 0 : min(max(R.carried, 0), 2 * W - 1);
  s.carry = carry + (long)R.slot * 2 * W;
  s.wav = wav + (long)R.src * ldw;
  s.first = R.fresh ? 0 : rs_first_input(R.out_before, U, D, W);
  s.carried = c;
  s.end = s.first + c + min(max(R.n_new, 0), max_new);
  return s;
}

// Outputs m0 .. m0 + cnt - 1 of `src` to out[0 .. cnt), zeros to out[cnt .. fill); cnt <= fill <= P K.  lds: the span.  Every
// thread of the workgroup calls it.  Output i of the tile: n0 = nfirst + dn, dn = (r0 + i D) / U, p = (r0 + i D) % U with
// (nfirst, r0) those of m0; outputs i and i + P have the same p and their dn differ by P D / U exactly.
template <bool STAGE, class Src>
__device__ __forceinline__ void resample_tile(const Src& src, const float* __restrict__ taps, int U, int D, int W, long m0, int cnt, int fill,
                                              float* __restrict__ out, float* lds, long cap, int P, int K) {
  const int tid = threadIdx.x, nt = blockDim.x, W2 = 2 * W;
  if (cnt <= 0) {
    for (int i = tid; i < fill; i += nt) out[i] = 0.f;
    return;
  }
  const unsigned long long q0 = (unsigned long long)m0 * (unsigned)D;
  const long nfirst = (long)(q0 / (unsigned)U);
  const unsigned r0 = (unsigned)(q0 % (unsigned)U);
  const long a0 = nfirst - W + 1;                                      // the clip position of span entry 0
  if constexpr (STAGE) {
    const unsigned long long ql = r0 + (unsigned long long)(cnt - 1) * (unsigned)D;
    const long span = min((long)(ql / (unsigned)U) + W2, cap);
    for (long i = tid; i < span; i += 8L * nt) {                        // eight loads in flight per thread: the staging is latency-bound
      float v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = i + (long)u * nt < span ? src.at(a0 + i + (long)u * nt) : 0.f;
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (i + (long)u * nt < span) lds[i + (long)u * nt] = v[u];
    }
    __syncthreads();
  }
  const long step = ((long)P * D) / U;
  auto X = [&](long o) { return STAGE ? lds[o] : src.at(a0 + o); };
  for (int ph = tid; ph < P && ph < fill; ph += nt) {
    const unsigned long long t = r0 + (unsigned long long)ph * (unsigned)D;
    unsigned long dn;
    unsigned p;
    if ((t >> 32) == 0) dn = (unsigned)t / (unsigned)U, p = (unsigned)t % (unsigned)U;
    else dn = t / (unsigned)U, p = (unsigned)(t % (unsigned)U);
    const float* hp = taps + (long)p * W2;                              // rows start on even floats: 8-byte aligned
    float acc[RS_K];
#pragma unroll
    for (int k = 0; k < RS_K; ++k) acc[k] = 0.f;
    int j = 0;
    for (; j + 8 <= W2; j += 8) {
      float h[8];
#pragma unroll
      for (int c = 0; c < 8; c += 2) {
        const float2 v = *reinterpret_cast<const float2*>(hp + j + c);
        h[c] = v.x, h[c + 1] = v.y;
      }
#pragma unroll
      for (int k = 0; k < RS_K; ++k) {
        if (k < K && ph + P * k < cnt) {
          const long o = (long)dn + k * step + j;
#pragma unroll
          for (int c = 0; c < 8; ++c) acc[k] = fmaf(h[c], X(o + c), acc[k]);
        }
      }
    }
    for (; j < W2; j += 2) {
      const float2 v = *reinterpret_cast<const float2*>(hp + j);
#pragma unroll
      for (int k = 0; k < RS_K; ++k) {
        if (k < K && ph + P * k < cnt) {
          const long o = (long)dn + k * step + j;
          acc[k] = fmaf(v.x, X(o), acc[k]);
          acc[k] = fmaf(v.y, X(o + 1), acc[k]);
        }
      }
    }
#pragma unroll
    for (int k = 0; k < RS_K; ++k) {
      const int i = ph + P * k;
      if (k < K && i < fill) out[i] = i < cnt ? acc[k] : 0.f;
    }
  }
}

template <bool STAGE>
__global__ void __launch_bounds__(RS_THREADS) k_resample(const float* __restrict__ wav, long ldw, const int* __restrict__ nsamp,
                                                         const float* __restrict__ taps, int U, int D, int W, float* __restrict__ out,
                                                         long ldo, int* __restrict__ nsamp_out, long cap, int P, int K) {
  extern __shared__ __align__(16) float rs_lds[];
  const int n = blockIdx.y, tile = P * K;
  const long n_in = min((long)max(nsamp[n], 0), ldw);
  const long olen = min(rs_cdiv(n_in * U, D), ldo);
  if (blockIdx.x == 0 && threadIdx.x == 0) nsamp_out[n] = (int)olen;
  const long m0 = (long)blockIdx.x * tile;
  const int fill = (int)min((long)tile, ldo - m0), cnt = (int)max(0L, min((long)fill, olen - m0));
  const ClipSrc src{wav + (long)n * ldw, n_in};
  resample_tile<STAGE>(src, taps, U, D, W, m0, cnt, fill, out + (long)n * ldo + m0, rs_lds, cap, P, K);
}

// grid (ntiles + 1, n_rows): workgroup x < ntiles computes tile x of row r's emit outputs (zeros up to max_emit); workgroup
// ntiles writes the samples the stream carries on, clip positions [first_input(out_before + emit), end), into ws[r][0 : 2W).
template <bool STAGE>
__global__ void __launch_bounds__(RS_THREADS) k_resample_stream(const float* __restrict__ wav, long ldw, const ResampleRow* __restrict__ rows,
                                                                int max_new, int max_emit, int S, const float* __restrict__ taps, int U,
                                                                int D, int W, const float* __restrict__ carry, float* __restrict__ out,
                                                                long ldo, float* __restrict__ ws, long cap, int P, int K, int ntiles) {
  extern __shared__ __align__(16) float rs_lds[];
  const int r = blockIdx.y, tile = P * K;
  const ResampleRow R = rows[r];
  if ((unsigned)R.slot >= (unsigned)S) return;
  const StreamSrc src = stream_src(R, carry, wav, ldw, max_new, U, D, W);
  const int emit = min(max(R.emit, 0), max_emit);
  if ((int)blockIdx.x == ntiles) {
    if (R.final_) return;
    const long from = rs_first_input(R.out_before + emit, U, D, W);
    const int keep = (int)min(max(src.end - from, 0L), 2L * W - 1);
    for (int k = threadIdx.x; k < keep; k += blockDim.x) ws[(long)r * 2 * W + k] = src.at(from + k);
    return;
  }
  const long i0 = (long)blockIdx.x * tile;
  const int fill = (int)min((long)tile, max_emit - i0), cnt = (int)max(0L, min((long)fill, emit - i0));
  resample_tile<STAGE>(src, taps, U, D, W, R.out_before + i0, cnt, fill, out + (long)r * ldo + i0, rs_lds, cap, P, K);
}

// grid (n_rows), 256 threads: ws[r][0 : keep) -> the slot's carry, keep as the launch before counted it
__global__ void __launch_bounds__(RS_THREADS) k_resample_stream_carry(const ResampleRow* __restrict__ rows, int max_new, int max_emit, int S,
                                                                      int U, int D, int W, const float* __restrict__ ws,
                                                                      float* __restrict__ carry) {
  const int r = blockIdx.x;
  const ResampleRow R = rows[r];
  if ((unsigned)R.slot >= (unsigned)S || R.final_) return;
  const int c = R.fresh ? 0 : min(max(R.carried, 0), 2 * W - 1), emit = min(max(R.emit, 0), max_emit);
  const long first = R.fresh ? 0 : rs_first_input(R.out_before, U, D, W);
  const long end = first + c + min(max(R.n_new, 0), max_new);
  const long from = rs_first_input(R.out_before + emit, U, D, W);
  const int keep = (int)min(max(end - from, 0L), 2L * W - 1);
  for (int k = threadIdx.x; k < keep; k += RS_THREADS) carry[(long)R.slot * 2 * W + k] = ws[(long)r * 2 * W + k];
}

}  // namespace

extern "C" {

// host-only queries: the output length of n input samples, the outputs one workgroup computes (tests place clip ends on its seams)
long ds2_resample_out_len(long n, int U, int D) { return n < 0 || U < 1 || D < 1 || n > (1L << 62) / U ? -1 : rs_cdiv(n * U, D); }
int ds2_resample_tile(int U, int D, int W) { return rs_shape_ok(U, D, W) ? rs_cfg(U, D, W).tile : -1; }

// Host only.  After samples_before input samples of a stream, a feed of n_new more (final != 0: the last of the utterance):
//   out[0] outputs that exist before the feed, out[1] outputs the feed emits, out[2] samples the feed takes from the carry,
//   out[3] samples carried on (at most 2W - 1; 0 after a final feed), out[4] the clip position of the first carried sample.
int ds2_resample_plan(long samples_before, int n_new, int final_, int U, int D, int W, long* out) {
  DS2_REQUIRE(out != nullptr && samples_before >= 0 && n_new >= 0 && samples_before <= (1L << 46) && rs_shape_ok(U, D, W), DS2_ERR_ARG);
  const long G0 = samples_before, G1 = G0 + n_new;
  const long e0 = rs_outputs(G0, 0, U, D, W), e1 = rs_outputs(G1, final_, U, D, W);
  const long first = rs_first_input(e0, U, D, W);
  out[0] = e0;
  out[1] = e1 - e0;
  out[2] = G0 - first;
  out[3] = final_ ? 0 : G1 - rs_first_input(e1, U, D, W);
  out[4] = first;
  return 0;
}

int ds2_resample(const float* wav, long ldw, const int* nsamples, int N, const float* taps, int U, int D, int W, float* out, long ldo,
                 int* nsamples_out, ds2_stream_t st_) {
  hipStream_t st = (hipStream_t)st_;
  DS2_REQUIRE(wav && nsamples && taps && out && nsamples_out && wav != out && N > 0 && N <= 65535 && ldw > 0 && ldo > 0, DS2_ERR_ARG);
  DS2_REQUIRE(rs_shape_ok(U, D, W), DS2_ERR_ARG);
  DS2_REQUIRE(((uintptr_t)taps & 7) == 0, DS2_ERR_ALIGN);
  const RsCfg c = rs_cfg(U, D, W);
  const long tiles = (ldo + c.tile - 1) / c.tile;
  DS2_REQUIRE(tiles <= 0x7fffffffL, DS2_ERR_ARG);
  const dim3 grid((unsigned)tiles, N), block(c.nt);
  if (c.cap == 0)
    hipLaunchKernelGGL(k_resample<false>, grid, block, c.lds, st, wav, ldw, nsamples, taps, U, D, W, out, ldo, nsamples_out, c.cap, c.P, c.K);
  else
    hipLaunchKernelGGL(k_resample<true>, grid, block, c.lds, st, wav, ldw, nsamples, taps, U, D, W, out, ldo, nsamples_out, c.cap, c.P, c.K);
  DS2_CHECK_LAUNCH();
  return 0;
}

// per slot the carried input samples, [S][2W] f32; the workspace holds the next carry of every row, [n_rows][2W] f32
long ds2_resample_stream_state_bytes(int S, int W) { return S > 0 && W > 0 ? (long)S * 2 * W * 4 : 0; }
long ds2_resample_stream_ws_bytes(int n_rows, int W) { return n_rows > 0 && W > 0 ? (long)n_rows * 2 * W * 4 : -1; }

int ds2_resample_stream_feed(const float* wav, long ldw, const ds2_resample_stream_row* rows, int n_rows, int max_new, int max_emit, int S,
                             const float* taps, int U, int D, int W, void* state, float* out, long ldo, void* ws, ds2_stream_t st_) {
  hipStream_t st = (hipStream_t)st_;
  static_assert(sizeof(ds2_resample_stream_row) == sizeof(ResampleRow), "row table layout");
  DS2_REQUIRE(rows && taps && state && ws && n_rows > 0 && n_rows <= 65535 && S >= n_rows && max_new >= 0 && max_emit >= 0, DS2_ERR_ARG);
  DS2_REQUIRE(((wav && ldw >= max_new) || max_new == 0) && ((out && ldo >= max_emit) || max_emit == 0), DS2_ERR_ARG);
  DS2_REQUIRE(rs_shape_ok(U, D, W), DS2_ERR_ARG);
  DS2_REQUIRE(((uintptr_t)rows & 7) == 0 && ((uintptr_t)taps & 7) == 0, DS2_ERR_ALIGN);
  RsCfg c = rs_cfg(U, D, W);
  // a feed is small: fewer outputs per thread, so that the rows together still bring ~256 workgroups (the sum does not depend on K)
  const int K = (int)std::min<long>(c.K, std::max<long>(1, ds2_cdiv(max_emit, (long)c.P * ds2_cdiv(256, n_rows))));
  if (K != c.K) {
    c.K = K, c.tile = c.P * K;
    if (c.cap) c.cap = rs_cap(c.P, K, U, D, W), c.lds = (size_t)c.cap * 4;
  }
  const int ntiles = (max_emit + c.tile - 1) / c.tile;
  const ResampleRow* R = (const ResampleRow*)rows;
  const dim3 grid(ntiles + 1, n_rows), block(c.nt);
  if (c.cap == 0)
    hipLaunchKernelGGL(k_resample_stream<false>, grid, block, c.lds, st, wav, ldw, R, max_new, max_emit, S, taps, U, D, W, (const float*)state,
                       out, ldo, (float*)ws, c.cap, c.P, c.K, ntiles);
  else
    hipLaunchKernelGGL(k_resample_stream<true>, grid, block, c.lds, st, wav, ldw, R, max_new, max_emit, S, taps, U, D, W, (const float*)state,
                       out, ldo, (float*)ws, c.cap, c.P, c.K, ntiles);
  DS2_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_resample_stream_carry, dim3(n_rows), dim3(RS_THREADS), 0, st, R, max_new, max_emit, S, U, D, W, (const float*)ws, (float*)state);
  DS2_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
