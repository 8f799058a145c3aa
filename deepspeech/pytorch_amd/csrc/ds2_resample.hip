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
// MIXED RATES: a class is one (U, D, W, taps) -- what the entries above take per launch; the _mixed entries take up to 16 in a
// device table (ds2_resample_class, filled on the host by ds2_resample_classes from rs_cfg) and one class index per row.
//   k_resample_mixed / k_resample_stream_mixed / k_resample_stream_carry_mixed : the kernels above with U, D, W, the table and
//                       the tile shape read from the row's class.  blockIdx.y is the row, so the class -- and with it staged span or
//                       global reads, 192 or 256 active threads, P, K -- is uniform over the workgroup: every thread reaches every
//                       barrier.  RS_THREADS threads are launched and the dynamic LDS is that of the largest class; grid.x is the
//                       tile count of the class with the smallest tile, and a workgroup beyond its own row's tiles returns at once.
//                       The tile body is the one above, so a row of a mixed launch is the row of a single-rate launch bit for bit.
//   The copy class U = D = 1, W = 0 has no table: y[m] = x[m], the bits as they are.  A class index outside [0, C) gives zeros.
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
  int emit, final_, fresh, cls;          // cls: the row's class in the _mixed entries (the header's pad word)
};

// ldc: floats between the carries of two slots (2W, or 2 Wmax of a bank)
__device__ __forceinline__ StreamSrc stream_src(const ResampleRow& R, const float* carry, long ldc, const float* wav, long ldw, int max_new,
                                                int U, int D, int W) {
  StreamSrc s;
  const int c = R.fresh ? 0 : min(max(R.carried, 0), 2 * W - 1);
  s.carry = carry + (long)R.slot * ldc;
  s.wav = wav + (long)R.src * ldw;
  s.first = R.fresh ? 0 : rs_first_input(R.out_before, U, D, W);
  s.carried = c;
  s.end = s.first + c + min(max(R.n_new, 0), max_new);
  return s;
}

// The samples row R's stream carries on, clip positions [first_input(out_before + emit), end), at most 2W - 1: src -> ws_row.
__device__ __forceinline__ void stream_keep(const ResampleRow& R, const StreamSrc& src, int emit, int U, int D, int W, float* __restrict__ ws_row) {
  if (R.final_) return;
  const long from = rs_first_input(R.out_before + emit, U, D, W);
  const int keep = (int)min(max(src.end - from, 0L), 2L * W - 1);
  for (int k = threadIdx.x; k < keep; k += blockDim.x) ws_row[k] = src.at(from + k);
}
// ws_row[0 : keep) -> the slot's carry, keep as stream_keep counted it in the launch before
__device__ __forceinline__ void stream_carry(const ResampleRow& R, int max_new, int max_emit, int U, int D, int W,
                                             const float* __restrict__ ws_row, float* __restrict__ carry_row) {
  if (R.final_) return;
  const int c = R.fresh ? 0 : min(max(R.carried, 0), 2 * W - 1), emit = min(max(R.emit, 0), max_emit);
  const long first = R.fresh ? 0 : rs_first_input(R.out_before, U, D, W);
  const long end = first + c + min(max(R.n_new, 0), max_new);
  const long from = rs_first_input(R.out_before + emit, U, D, W);
  const int keep = (int)min(max(end - from, 0L), 2L * W - 1);
  for (int k = threadIdx.x; k < keep; k += blockDim.x) carry_row[k] = ws_row[k];
}

// Outputs m0 .. m0 + cnt - 1 of `src` to out[0 .. cnt), zeros to out[cnt .. fill); cnt <= fill <= P K.  lds: the span.  Every
// thread of the workgroup calls it and reaches the barrier.  nt: the threads that work -- blockDim.x, or with PART the first nt of
// them (a mixed launch has RS_THREADS threads whatever the class).  Output i of the tile: n0 = nfirst + dn, dn = (r0 + i D) / U, p = (r0 + i D) % U with
// (nfirst, r0) those of m0; outputs i and i + P have the same p and their dn differ by P D / U exactly.
template <bool STAGE, bool PART, class Src>
__device__ __forceinline__ void resample_tile(const Src& src, const float* __restrict__ taps, int U, int D, int W, long m0, int cnt, int fill,
                                              float* __restrict__ out, float* lds, long cap, int P, int K, int nt) {
  const int tid = threadIdx.x, W2 = 2 * W;
  const bool idle = PART && tid >= nt;
  if (cnt <= 0) {
    for (int i = idle ? fill : tid; i < fill; i += nt) out[i] = 0.f;
    return;
  }
  const unsigned long long q0 = (unsigned long long)m0 * (unsigned)D;
  const long nfirst = (long)(q0 / (unsigned)U);
  const unsigned r0 = (unsigned)(q0 % (unsigned)U);
  const long a0 = nfirst - W + 1;                                      // the clip position of span entry 0
  if constexpr (STAGE) {
    const unsigned long long ql = r0 + (unsigned long long)(cnt - 1) * (unsigned)D;
    const long span = min((long)(ql / (unsigned)U) + W2, cap);
    for (long i = idle ? span : tid; i < span; i += 8L * nt) {                        // eight loads in flight per thread: the staging is latency-bound
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
  for (int ph = idle ? P : tid; ph < P && ph < fill; ph += nt) {
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
  resample_tile<STAGE, false>(src, taps, U, D, W, m0, cnt, fill, out + (long)n * ldo + m0, rs_lds, cap, P, K, blockDim.x);
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
  const StreamSrc src = stream_src(R, carry, 2L * W, wav, ldw, max_new, U, D, W);
  const int emit = min(max(R.emit, 0), max_emit);
  if ((int)blockIdx.x == ntiles) {
    stream_keep(R, src, emit, U, D, W, ws + (long)r * 2 * W);
    return;
  }
  const long i0 = (long)blockIdx.x * tile;
  const int fill = (int)min((long)tile, max_emit - i0), cnt = (int)max(0L, min((long)fill, emit - i0));
  resample_tile<STAGE, false>(src, taps, U, D, W, R.out_before + i0, cnt, fill, out + (long)r * ldo + i0, rs_lds, cap, P, K, blockDim.x);
}

// grid (n_rows), 256 threads: ws[r][0 : keep) -> the slot's carry, keep as the launch before counted it
__global__ void __launch_bounds__(RS_THREADS) k_resample_stream_carry(const ResampleRow* __restrict__ rows, int max_new, int max_emit, int S,
                                                                      int U, int D, int W, const float* __restrict__ ws,
                                                                      float* __restrict__ carry) {
  const int r = blockIdx.x;
  const ResampleRow R = rows[r];
  if ((unsigned)R.slot >= (unsigned)S) return;
  stream_carry(R, max_new, max_emit, U, D, W, ws + (long)r * 2 * W, carry + (long)R.slot * 2 * W);
}

// ---- mixed rates: U, D, W, the table and the tile shape belong to the row's class -----------------------------------------------
// One class of the device table (ds2_resample_class of include/ds2hip.h)
struct RsClass {
  int U, D, W;             // 1, 1, 0: the copy class
  int nt, P, K, tile;      // rs_cfg's shape (the copy class: RS_THREADS, RS_THREADS, RS_K)
  int cap;                 // floats of the staged span, 0 = the input is read from global memory
  long long taps_off;      // floats in front of the class's table in the taps buffer, even
};
constexpr int RS_CLASSES_MAX = 16;

inline bool rs_is_copy(int U, int D, int W) { return U == 1 && D == 1 && W == 0; }

// a feed is small: fewer outputs per thread, so that the rows together still bring ~256 workgroups (the sum does not depend on K)
__host__ __device__ inline int rs_stream_k(int K, int P, int max_emit, int n_rows) {
  const long k = rs_cdiv(max_emit, (long)P * rs_cdiv(256, n_rows));
  return (int)(k < 1 ? 1 : k < K ? k : K);
}

// The class's tile body: the branch is uniform over the workgroup.  GLOBAL: the table has a class without a staged span.  The
// body that reads the input from global memory keeps 16 x 8 loads in flight and takes 284 VGPRs against the staged body's 50 --
// one workgroup per CU instead of three -- so the entries launch the kernel that contains it only for a table that needs it.
template <bool GLOBAL, class Src>
__device__ __forceinline__ void resample_tile_class(const Src& src, const RsClass& c, int K, const float* __restrict__ taps, long m0, int cnt,
                                                    int fill, float* __restrict__ out, float* lds) {
  if (!GLOBAL || c.cap) resample_tile<true, true>(src, taps + c.taps_off, c.U, c.D, c.W, m0, cnt, fill, out, lds, c.cap, c.P, K, c.nt);
  else resample_tile<false, true>(src, taps + c.taps_off, c.U, c.D, c.W, m0, cnt, fill, out, lds, c.cap, c.P, K, c.nt);
}
// the copy class: x[0 .. cnt) -> out[0 .. cnt), zeros to out[cnt .. fill)
__device__ __forceinline__ void copy_tile(const float* __restrict__ x, int cnt, int fill, float* __restrict__ out) {
  for (int i = threadIdx.x; i < fill; i += blockDim.x) out[i] = i < cnt ? x[i] : 0.f;
}

// grid (ceil(ldo / ztile), N), RS_THREADS threads, ztile = the smallest tile of the table: workgroup x computes tile x of ITS
// row's class and returns when the row has no such tile.  A row whose class is outside [0, C): zeros in tiles of ztile, count 0.
template <bool GLOBAL>
__global__ void __launch_bounds__(RS_THREADS) k_resample_mixed(const float* __restrict__ wav, long ldw, const int* __restrict__ nsamp,
                                                               const int* __restrict__ cls, const RsClass* __restrict__ classes, int C,
                                                               int ztile, const float* __restrict__ taps, float* __restrict__ out, long ldo,
                                                               int* __restrict__ nsamp_out) {
  extern __shared__ __align__(16) float rs_lds[];
  const int n = blockIdx.y, c = cls[n];
  const bool known = (unsigned)c < (unsigned)C;
  RsClass k;
  if (known) k = classes[c];
  const int tile = known ? k.tile : ztile;
  const long m0 = (long)blockIdx.x * tile;
  if (m0 >= ldo) return;
  const int fill = (int)min((long)tile, ldo - m0);
  float* o = out + (long)n * ldo + m0;
  if (!known) {
    if (blockIdx.x == 0 && threadIdx.x == 0) nsamp_out[n] = 0;
    copy_tile(nullptr, 0, fill, o);
    return;
  }
  const long n_in = min((long)max(nsamp[n], 0), ldw);
  const long olen = min(k.W == 0 ? n_in : rs_cdiv(n_in * k.U, k.D), ldo);
  if (blockIdx.x == 0 && threadIdx.x == 0) nsamp_out[n] = (int)olen;
  const int cnt = (int)max(0L, min((long)fill, olen - m0));
  if (k.W == 0) {
    copy_tile(wav + (long)n * ldw + m0, cnt, fill, o);
    return;
  }
  const ClipSrc src{wav + (long)n * ldw, n_in};
  resample_tile_class<GLOBAL>(src, k, k.K, taps, m0, cnt, fill, o, rs_lds);
}

// grid (ntiles + 1, n_rows), RS_THREADS threads, ntiles = ceil(max_emit / ztile): k_resample_stream per row's class (R.cls); the
// carries of two slots lie 2 Wmax floats apart, and so do the rows of ws.  The copy class carries nothing.
template <bool GLOBAL>
__global__ void __launch_bounds__(RS_THREADS) k_resample_stream_mixed(const float* __restrict__ wav, long ldw,
                                                                      const ResampleRow* __restrict__ rows, int n_rows, int max_new,
                                                                      int max_emit, int S, const RsClass* __restrict__ classes, int C,
                                                                      int ztile, const float* __restrict__ taps,
                                                                      const float* __restrict__ carry, int Wmax, float* __restrict__ out,
                                                                      long ldo, float* __restrict__ ws, int ntiles) {
  extern __shared__ __align__(16) float rs_lds[];
  const int r = blockIdx.y;
  const ResampleRow R = rows[r];
  if ((unsigned)R.slot >= (unsigned)S) return;
  const bool known = (unsigned)R.cls < (unsigned)C, last = (int)blockIdx.x == ntiles;
  if (!known && last) return;
  RsClass k;
  int K = 1;
  if (known) k = classes[R.cls], K = rs_stream_k(k.K, k.P, max_emit, n_rows);
  const int tile = known ? k.P * K : ztile;
  const int emit = known ? min(max(R.emit, 0), max_emit) : 0;
  const long i0 = (long)blockIdx.x * tile;
  if (!last && i0 >= max_emit) return;
  const int fill = (int)min((long)tile, max_emit - i0), cnt = (int)max(0L, min((long)fill, emit - i0));
  float* o = out + (long)r * ldo + i0;
  if (!known || k.W == 0) {
    if (last) return;
    const int n_new = min(max(R.n_new, 0), max_new);
    copy_tile(known ? wav + (long)R.src * ldw + i0 : nullptr, known ? (int)max(0L, min((long)cnt, n_new - i0)) : 0, fill, o);
    return;
  }
  const StreamSrc src = stream_src(R, carry, 2L * Wmax, wav, ldw, max_new, k.U, k.D, k.W);
  if (last) {
    stream_keep(R, src, emit, k.U, k.D, k.W, ws + (long)r * 2 * Wmax);
    return;
  }
  resample_tile_class<GLOBAL>(src, k, K, taps, R.out_before + i0, cnt, fill, o, rs_lds);
}

// grid (n_rows), RS_THREADS threads
__global__ void __launch_bounds__(RS_THREADS) k_resample_stream_carry_mixed(const ResampleRow* __restrict__ rows, int max_new, int max_emit,
                                                                            int S, const RsClass* __restrict__ classes, int C, int Wmax,
                                                                            const float* __restrict__ ws, float* __restrict__ carry) {
  const int r = blockIdx.x;
  const ResampleRow R = rows[r];
  if ((unsigned)R.slot >= (unsigned)S || (unsigned)R.cls >= (unsigned)C) return;
  const RsClass k = classes[R.cls];
  if (k.W == 0) return;
  stream_carry(R, max_new, max_emit, k.U, k.D, k.W, ws + (long)r * 2 * Wmax, carry + (long)R.slot * 2 * Wmax);
}

// the host's copy of a class table, checked: 0, or the error code
inline int rs_classes_ok(const RsClass* cl, int C) {
  DS2_REQUIRE(cl != nullptr && C >= 1 && C <= RS_CLASSES_MAX, DS2_ERR_ARG);
  for (int c = 0; c < C; ++c) {
    const RsClass& k = cl[c];
    if (rs_is_copy(k.U, k.D, k.W)) {
      DS2_REQUIRE(k.nt == RS_THREADS && k.P == RS_THREADS && k.K == RS_K && k.tile == RS_THREADS * RS_K && k.cap == 0, DS2_ERR_ARG);
      continue;
    }
    DS2_REQUIRE(rs_shape_ok(k.U, k.D, k.W) && k.taps_off >= 0, DS2_ERR_ARG);
    const RsCfg g = rs_cfg(k.U, k.D, k.W);
    DS2_REQUIRE(k.nt == g.nt && k.P == g.P && k.K == g.K && k.tile == g.tile && k.cap == g.cap, DS2_ERR_ARG);
    DS2_REQUIRE((k.taps_off & 1) == 0, DS2_ERR_ALIGN);
  }
  return 0;
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
  const int K = rs_stream_k(c.K, c.P, max_emit, n_rows);
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

// ---- mixed rates --------------------------------------------------------------------------------------------------------------
// Host only.  udw [C][3] = (U, D, W) per class -> table [C] (the caller uploads the same bytes as the device table) and
// taps_floats = the floats of the taps buffer: class c's table [U][2W] lies taps_off floats in, the tables one behind the other
// (2W floats a row: every one starts 8-byte aligned).  (1, 1, 0) is the copy class: no table.
int ds2_resample_classes(const int* udw, int C, ds2_resample_class* table, long* taps_floats) {
  static_assert(sizeof(ds2_resample_class) == sizeof(RsClass), "class table layout");
  DS2_REQUIRE(udw && table && taps_floats && C >= 1 && C <= RS_CLASSES_MAX, DS2_ERR_ARG);
  for (int c = 0; c < C; ++c)
    DS2_REQUIRE(rs_is_copy(udw[3 * c], udw[3 * c + 1], udw[3 * c + 2]) || rs_shape_ok(udw[3 * c], udw[3 * c + 1], udw[3 * c + 2]), DS2_ERR_ARG);
  RsClass* t = (RsClass*)table;
  long off = 0;
  for (int c = 0; c < C; ++c) {
    const int U = udw[3 * c], D = udw[3 * c + 1], W = udw[3 * c + 2];
    if (rs_is_copy(U, D, W)) {
      t[c] = RsClass{1, 1, 0, RS_THREADS, RS_THREADS, RS_K, RS_THREADS * RS_K, 0, off};
      continue;
    }
    const RsCfg g = rs_cfg(U, D, W);
    t[c] = RsClass{U, D, W, g.nt, g.P, g.K, g.tile, (int)g.cap, off};
    off += (long)U * 2 * W;
  }
  *taps_floats = off;
  return 0;
}

// classes: the host's table as ds2_resample_classes filled it, classes_dev: the same bytes on the device
int ds2_resample_mixed(const float* wav, long ldw, const int* nsamples, const int* cls, int N, const ds2_resample_class* classes,
                       const ds2_resample_class* classes_dev, int C, const float* taps, float* out, long ldo, int* nsamples_out,
                       ds2_stream_t st_) {
  hipStream_t st = (hipStream_t)st_;
  const RsClass* cl = (const RsClass*)classes;
  DS2_REQUIRE(wav && nsamples && cls && classes_dev && out && nsamples_out && wav != out && N > 0 && N <= 65535 && ldw > 0 && ldo > 0,
              DS2_ERR_ARG);
  if (const int e = rs_classes_ok(cl, C)) return e;
  int ztile = cl[0].tile;
  size_t lds = 0;
  bool tables = false, global = false;
  for (int c = 0; c < C; ++c) {
    ztile = std::min(ztile, cl[c].tile), lds = std::max(lds, (size_t)cl[c].cap * 4);
    tables = tables || cl[c].W > 0, global = global || (cl[c].W > 0 && cl[c].cap == 0);
  }
  DS2_REQUIRE(taps || !tables, DS2_ERR_ARG);
  DS2_REQUIRE(((uintptr_t)taps & 7) == 0 && ((uintptr_t)classes_dev & 7) == 0, DS2_ERR_ALIGN);
  const long tiles = (ldo + ztile - 1) / ztile;
  DS2_REQUIRE(tiles <= 0x7fffffffL, DS2_ERR_ARG);
  hipLaunchKernelGGL(global ? k_resample_mixed<true> : k_resample_mixed<false>, dim3((unsigned)tiles, N), dim3(RS_THREADS), lds, st, wav, ldw,
                     nsamples, cls, (const RsClass*)classes_dev, C, ztile, taps, out, ldo, nsamples_out);
  DS2_CHECK_LAUNCH();
  return 0;
}

// [S][2 Wmax] f32 and [n_rows][2 Wmax] f32, Wmax = the largest W of the bank (a bank of the copy class alone: 1)
long ds2_resample_stream_state_bytes_mixed(int S, int Wmax) { return ds2_resample_stream_state_bytes(S, Wmax); }
long ds2_resample_stream_ws_bytes_mixed(int n_rows, int Wmax) { return ds2_resample_stream_ws_bytes(n_rows, Wmax); }

int ds2_resample_stream_feed_mixed(const float* wav, long ldw, const ds2_resample_stream_row* rows, int n_rows, int max_new, int max_emit,
                                   int S, const ds2_resample_class* classes, const ds2_resample_class* classes_dev, int C, const float* taps,
                                   int Wmax, void* state, float* out, long ldo, void* ws, ds2_stream_t st_) {
  hipStream_t st = (hipStream_t)st_;
  const RsClass* cl = (const RsClass*)classes;
  DS2_REQUIRE(rows && classes_dev && state && ws && n_rows > 0 && n_rows <= 65535 && S >= n_rows && max_new >= 0 && max_emit >= 0 && Wmax >= 1,
              DS2_ERR_ARG);
  DS2_REQUIRE(((wav && ldw >= max_new) || max_new == 0) && ((out && ldo >= max_emit) || max_emit == 0) && (wav != out || !wav), DS2_ERR_ARG);
  if (const int e = rs_classes_ok(cl, C)) return e;
  int ztile = 0;
  size_t lds = 0;
  bool tables = false, global = false;
  for (int c = 0; c < C; ++c) {
    const RsClass& k = cl[c];
    DS2_REQUIRE(k.W <= Wmax, DS2_ERR_ARG);
    const int K = rs_stream_k(k.K, k.P, max_emit, n_rows);
    ztile = c == 0 ? k.P * K : std::min(ztile, k.P * K);
    if (k.cap) lds = std::max(lds, (size_t)rs_cap(k.P, K, k.U, k.D, k.W) * 4);
    tables = tables || k.W > 0, global = global || (k.W > 0 && k.cap == 0);
  }
  DS2_REQUIRE(taps || !tables, DS2_ERR_ARG);
  DS2_REQUIRE(((uintptr_t)rows & 7) == 0 && ((uintptr_t)taps & 7) == 0 && ((uintptr_t)classes_dev & 7) == 0, DS2_ERR_ALIGN);
  const int ntiles = (max_emit + ztile - 1) / ztile;
  const ResampleRow* R = (const ResampleRow*)rows;
  const RsClass* cd = (const RsClass*)classes_dev;
  hipLaunchKernelGGL(global ? k_resample_stream_mixed<true> : k_resample_stream_mixed<false>, dim3(ntiles + 1, n_rows), dim3(RS_THREADS), lds, st,
                     wav, ldw, R, n_rows, max_new, max_emit, S, cd, C, ztile, taps, (const float*)state, Wmax, out, ldo, (float*)ws, ntiles);
  DS2_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_resample_stream_carry_mixed, dim3(n_rows), dim3(RS_THREADS), 0, st, R, max_new, max_emit, S, cd, C, Wmax, (const float*)ws,
                     (float*)state);
  DS2_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
