// Exact chunked inference: the conv front-end and the lookahead with their time context carried from
// feed to feed, so that a uni-directional model in eval mode gives, chunk after chunk, the frames of the one-shot forward.
//
// All three kernels read a per-stream VIRTUAL WINDOW over time:   position i <  K           the carry buffer (the K positions
//                                                                                            in front of this feed's chunk)
//                                                                 K <= i < K + len[n]       the chunk
//                                                                 anything else             0
// and write, besides their outputs, the NEXT carry next[i] = V[len + i] (i < K) into a second buffer: the old carry is read
// while the new one is written, so the session ping-pongs two buffers.  Output frame j of a launch reads the window from
// position off + stride * j on; frames j >= live[n] are written as zeros (MaskConv's mask at the end of an utterance).
//
//   k_stream_conv1      Conv2d(1,32,(41,11),s=(2,2)) + eval BatchNorm2d + Hardtanh(0,20); the tile body of k_conv1_fwd (ds2_conv.hip)
//   k_stream_conv2      Conv2d(32,32,(21,11),s=(2,1)) + eval BatchNorm2d + Hardtanh(0,20) on MFMA; the tile body of k_conv_tap<T, 1>;
//                       writes the sequence layout X0[(j*N + n)][rld] the recurrent stack reads
//   k_stream_lookahead  hardtanh(sum_k w[h][k] * V[t + k]); taps ascending with fmaf, as k_lookahead_fwd (ds2_seqops.hip)
// Shapes are small (1..32 streams, a few to ~100 frames a feed): one short launch each, no persistent loops.
//
// Every kernel has a second instantiation, ROWS, for a pool of streams that each follow their own plan:
// one ds2_stream_row per batch row gives the carry slot, the row of x, which of the two carry buffers holds the slot's carry
// (per stage), whether that carry reads as zero (a stream's first feed) and the row's own len / off / cnt of every stage.  The
// tile bodies, the fmaf order and the epilogues are shared, so a pool in lock step computes what the un-tabled kernels compute.
#include "ds2_common.h"

namespace {

constexpr int CH = 32;
constexpr int K1F = 41, K1T = 11, K2F = 21, K2T = 11;
constexpr int SK = 10;                                     // carried positions of both convolutions (kernel width - 1)

// ============================================================================================================
// conv1 over the window [carry 10 input frames | chunk]
// ============================================================================================================
constexpr int C1_FB = 4, C1_TB = 64;                       // output tile: 4 freq rows x 64 frames
constexpr int C1_PR = (C1_FB - 1) * 2 + K1F;               // 47 input rows
constexpr int C1_PC = (C1_TB - 1) * 2 + K1T;               // 137 input cols
constexpr int C1_PCP = C1_PC + 1;

// ROWS: carry / next are the two buffers [S][F0][10] of the pool, the row's slot is read from one and written into the other
template <typename T, bool ROWS>
__global__ void __launch_bounds__(256) k_stream_conv1(const float* __restrict__ x, const float* __restrict__ carry,
                                                       float* __restrict__ next, const float* __restrict__ w1k,
                                                       const float* __restrict__ b1, const float* __restrict__ scale,
                                                       const float* __restrict__ shift, const int* __restrict__ len,
                                                       const int* __restrict__ live, T* __restrict__ y, int N, int Tc, int off, int J,
                                                       int f0, int f1, int ntiles, const ds2_stream_row* __restrict__ rows) {
  __shared__ float patch[C1_PR * C1_PCP];
  const int tid = threadIdx.x, n = blockIdx.z;
  int ln, nlive = 0;                                 // ROWS: the row's own count of output frames
  bool fresh = false;
  const float *xn, *cn;
  float* nn;
  if constexpr (ROWS) {
    const ds2_stream_row R = rows[n];
    const bool cur = (R.cur & 1) != 0;
    ln = min(max(R.len, 0), Tc);
    off = R.off1;
    nlive = R.cnt1;
    fresh = (R.fresh & 1) != 0;
    xn = x + (long)R.src * f0 * Tc;
    cn = (cur ? (const float*)next : carry) + (long)R.slot * f0 * SK;
    nn = (cur ? const_cast<float*>(carry) : next) + (long)R.slot * f0 * SK;
  } else {
    ln = len ? min(max(len[n], 0), Tc) : Tc;
    xn = x + (long)n * f0 * Tc;
    cn = carry + (long)n * f0 * SK;
    nn = next + (long)n * f0 * SK;
  }
  if ((int)blockIdx.x == ntiles) {
    // the carry blocks: rows [r0, r1) of this stream, next[f][i] = V[f][ln + i]
    const int per = ds2_cdiv_dev(f0, gridDim.y);
    const int r0 = blockIdx.y * per, r1 = min(r0 + per, f0);
    for (int e = r0 * SK + tid; e < r1 * SK; e += 256) {
      const int f = e / SK, p = ln + (e - f * SK);        // p < SK + ln always
      nn[e] = p < SK ? (fresh ? 0.f : cn[f * SK + p]) : xn[(long)f * Tc + (p - SK)];
    }
    return;
  }
  const int to0 = blockIdx.x * C1_TB, fo0 = blockIdx.y * C1_FB;
  const int f_base = 2 * fo0 - 20, p_base = off + 2 * to0;
  for (int i = tid; i < C1_PR * C1_PC; i += 256) {
    const int pr = i / C1_PC, pc = i - pr * C1_PC;
    const int fi = f_base + pr, p = p_base + pc;
    const int fc = min(max(fi, 0), f0 - 1);
    // unconditional load from an address that always exists (the carry's when the position is not in the chunk), zeroed by a
    // select afterwards: keeps all of a thread's ~25 loads in flight
    const bool inx = p >= SK && p < SK + ln;
    const bool ok = fi >= 0 && fi < f0 && p >= 0 && ((p < SK && !fresh) || inx);
    const float* src = inx ? xn + (long)fc * Tc + (p - SK) : cn + fc * SK + min(max(p, 0), SK - 1);
    const float v = *src;
    patch[pr * C1_PCP + pc] = ok ? v : 0.f;
  }
  __syncthreads();
  const int r = tid >> 6, c = tid & 63;
  const int fo = fo0 + r, to = to0 + c;
  float acc[CH];
#pragma unroll
  for (int co = 0; co < CH; ++co) acc[co] = b1[co];
  const float* prow = patch + (2 * r) * C1_PCP + 2 * c;
  for (int kf = 0; kf < K1F; ++kf) {
    const float* wk = w1k + kf * K1T * CH;
#pragma unroll
    for (int kt = 0; kt < K1T; ++kt) {
      const float xv = prow[kf * C1_PCP + kt];
#pragma unroll
      for (int co = 0; co < CH; ++co) acc[co] = fmaf(xv, wk[kt * CH + co], acc[co]);
    }
  }
  if (fo < f1 && to < J) {
    const bool lv = ROWS ? to < nlive : (live ? (to < live[n]) : true);
    T* dst = y + (((long)n * f1 + fo) * J + to) * CH;
    constexpr int V = Vec16<T>::N;
#pragma unroll
    for (int v = 0; v < CH / V; ++v) {
      float o[V];
#pragma unroll
      for (int i = 0; i < V; ++i) {
        const int co = v * V + i;
        const float a = fminf(fmaxf(fmaf(acc[co], scale[co], shift[co]), 0.f), 20.f);      // eval BatchNorm2d + Hardtanh(0, 20)
        o[i] = lv ? a : 0.f;
      }
      Vec16<T>::store(dst + v * V, o);
    }
  }
}

// ============================================================================================================
// conv2 over the window [carry 10 activation frames | new activation frames]: MFMA tap-GEMM (k_conv_tap<T, 1>)
// ============================================================================================================
constexpr int CT_UB = 4, CT_TB = 32;          // output tile: 4 rows (one per wave) x 32 positions
constexpr int CT_POSB = 80;                   // LDS bytes per position / per weight row: 64 data + 16 pad
constexpr int CT_PR = (CT_UB - 1) * 2 + K2F;      // 27
constexpr int CT_PC = CT_TB + K2T - 1;            // 42
constexpr int CT_PATCH_BYTES = CT_PR * CT_PC * CT_POSB;          // 90720
constexpr int CT_WST_BYTES = K2T * CH * CT_POSB;                  // 28160 per kernel row (one pass)
constexpr int CT_SMEM = CT_PATCH_BYTES + 2 * CT_WST_BYTES;        // 147040

struct StreamConv2Args {
  const void* A;       // [N][F1][Jin][32] the new activation frames
  const void* carry;   // [N][F1][10][32]
  void* next;          // [N][F1][10][32]
  const void* W;       // [21*11][32 m][32 k]
  const float *bias, *scale, *shift;   // [32]
  const int *len, *live;               // [N] or null
  void* X0;            // [(j*N + n)][rld]
  int N, Jin, off, J, F1, F2, rld;
  const ds2_stream_row* rows;          // ROWS: carry / next are the pool's two buffers [S][F1][10][32]; X0 [(j*nrnn + n)][rld]
  int nrnn;                            //       holds the rows n < nrnn, the rows behind them only move their carry
};

template <typename T, bool ROWS>
__global__ void __launch_bounds__(256, 1) k_stream_conv2(StreamConv2Args a, int ntiles) {
  constexpr int V = Vec16<T>::N;
  constexpr int NPASS = (CH * (int)sizeof(T)) / 64;   // bf16: 1 pass of 32 channels; f32: 2 passes of 16 channels
  constexpr int CPB = 64 / (int)sizeof(T);            // channels per pass
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 31, lq = lane >> 5;
  const int n = blockIdx.z;
  int ln, off = a.off, nlive = 0, NR = a.N;         // nlive (ROWS): the row's own count of output frames
  uint32_t cmask = 0xffffffffu;                       // 0: the carry reads as zero
  const T* An = (const T*)a.A + (long)n * a.F1 * a.Jin * CH;
  const T* Cn;
  T* Nn;
  if constexpr (ROWS) {
    const ds2_stream_row R = a.rows[n];
    const bool cur = (R.cur & 2) != 0;
    ln = min(max(R.cnt1, 0), a.Jin);
    off = R.off2;
    nlive = R.cnt2;
    NR = a.nrnn;
    cmask = (R.fresh & 2) ? 0u : 0xffffffffu;
    Cn = (const T*)(cur ? a.next : a.carry) + (long)R.slot * a.F1 * SK * CH;
    Nn = (T*)(cur ? const_cast<void*>(a.carry) : a.next) + (long)R.slot * a.F1 * SK * CH;
  } else {
    ln = a.len ? min(max(a.len[n], 0), a.Jin) : a.Jin;
    Cn = (const T*)a.carry + (long)n * a.F1 * SK * CH;
    Nn = (T*)a.next + (long)n * a.F1 * SK * CH;
  }
  if ((int)blockIdx.x == ntiles) {
    // the carry blocks: rows [r0, r1) of this stream, 16-byte pieces of next[f][i][32] = V[f][ln + i][32]
    constexpr int PV = CH / V;                        // pieces per position
    const int per = ds2_cdiv_dev(a.F1, gridDim.y);
    const int r0 = blockIdx.y * per, r1 = min(r0 + per, a.F1);
    for (int e = r0 * SK * PV + tid; e < r1 * SK * PV; e += 256) {
      const int v = e % PV, pos = e / PV;
      const int f = pos / SK, p = ln + (pos - f * SK);
      const T* src = p < SK ? Cn + ((long)f * SK + p) * CH : An + ((long)f * a.Jin + (p - SK)) * CH;
      uint4 val = *reinterpret_cast<const uint4*>(src + v * V);
      if constexpr (ROWS) {
        const uint32_t m = p < SK ? cmask : 0xffffffffu;
        val.x &= m; val.y &= m; val.z &= m; val.w &= m;
      }
      *reinterpret_cast<uint4*>(Nn + (long)pos * CH + v * V) = val;
    }
    return;
  }
  if (ROWS && n >= NR) return;                       // no RNN frame this feed: the carry block above was this row's whole work
  const int to0 = blockIdx.x * CT_TB, u0 = blockIdx.y * CT_UB;
  unsigned char* patch = smem;
  unsigned char* wst = smem + CT_PATCH_BYTES;
  const int fi0 = u0 * 2 - 10, p0 = off + to0;
  const T* Wg = (const T*)a.W;

  ds2_f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;

  for (int pass = 0; pass < NPASS; ++pass) {
    const int c0 = pass * CPB;
    __syncthreads();   // previous pass finished reading patch / wst
    // ---- stage the input patch: 27 x 42 positions x 64 bytes
    for (int i = tid; i < CT_PR * CT_PC * 4; i += 256) {
      const int v = i & 3, pos = i >> 2;
      const int pr = pos / CT_PC, pc = pos - pr * CT_PC;
      const int fi = fi0 + pr, p = p0 + pc;
      // unconditional load from an address that always exists + bit mask (see k_conv_tap)
      const bool inx = p >= SK && p < SK + ln;
      uint32_t m = (fi >= 0 && fi < a.F1 && p >= 0 && (p < SK || inx)) ? 0xffffffffu : 0u;
      if constexpr (ROWS) m &= inx ? 0xffffffffu : cmask;
      const int fc = min(max(fi, 0), a.F1 - 1);
      const T* src = inx ? An + ((long)fc * a.Jin + (p - SK)) * CH : Cn + ((long)fc * SK + min(max(p, 0), SK - 1)) * CH;
      uint4 val = *reinterpret_cast<const uint4*>(src + c0 + v * V);
      val.x &= m; val.y &= m; val.z &= m; val.w &= m;
      *reinterpret_cast<uint4*>(patch + pos * CT_POSB + v * 16) = val;
    }
    // ---- weights of kernel row 0 of this pass
    auto wload = [&](int kf, int buf) {
      for (int i = tid; i < K2T * CH * 4; i += 256) {
        const int v = i & 3, row = i >> 2;   // row = kt*32 + m
        const uint4 val = *reinterpret_cast<const uint4*>(Wg + ((long)(kf * K2T) * CH + row) * CH + c0 + v * V);
        *reinterpret_cast<uint4*>(wst + buf * CT_WST_BYTES + row * CT_POSB + v * 16) = val;
      }
    };
    wload(0, 0);
    __syncthreads();
    for (int kf = 0; kf < K2F; ++kf) {
      const int buf = kf & 1;
      if (kf + 1 < K2F) wload(kf + 1, buf ^ 1);   // other buffer: last read two iterations ago (barrier in between)
      const unsigned char* wb = wst + buf * CT_WST_BYTES + li * CT_POSB + lq * 16;
      const unsigned char* pb = patch + ((wave * 2 + kf) * CT_PC + li) * CT_POSB + lq * 16;
#pragma unroll
      for (int kt = 0; kt < K2T; ++kt) {
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          const uint4 af = *reinterpret_cast<const uint4*>(wb + kt * CH * CT_POSB + c * 32);
          const uint4 bf = *reinterpret_cast<const uint4*>(pb + kt * CT_POSB + c * 32);
          Mma<T>::mma32(acc, af, bf);
        }
      }
      __syncthreads();
    }
  }

  // ---- epilogue: transpose the wave's [32 m][32 pos] tile through LDS, then 16 channels of one position per lane into X0
  float* tile = reinterpret_cast<float*>(smem) + wave * (32 * 33);
#pragma unroll
  for (int r = 0; r < 16; ++r) tile[li * 33 + mma32_row(r, lane)] = acc[r];   // tile[pos][m]
  __syncthreads();
  const int u = u0 + wave;
  const int pos = lane >> 1, half = lane & 1;
  const int to = to0 + pos;
  if (u < a.F2 && to < a.J) {
    const bool lv = ROWS ? to < nlive : (a.live ? (to < a.live[n]) : true);
    T* row = (T*)a.X0 + ((long)to * NR + n) * a.rld;
    T* dst = row + u * CH + half * 16;
#pragma unroll
    for (int v = 0; v < 16 / V; ++v) {
      float o[V];
#pragma unroll
      for (int i = 0; i < V; ++i) {
        const int m = half * 16 + v * V + i;
        const float val = fminf(fmaxf(fmaf(tile[pos * 33 + m] + a.bias[m], a.scale[m], a.shift[m]), 0.f), 20.f);
        o[i] = lv ? val : 0.f;
      }
      Vec16<T>::store(dst + v * V, o);
    }
    if (u == a.F2 - 1) {               // the zero pad columns of the sequence layout (up to the GEMM K-tile)
      float z[V];
#pragma unroll
      for (int i = 0; i < V; ++i) z[i] = 0.f;
      for (int c = a.F2 * CH + half * 16; c + 16 <= a.rld; c += 32)
#pragma unroll
        for (int v = 0; v < 16 / V; ++v) Vec16<T>::store(row + c + v * V, z);
    }
  }
}

// ============================================================================================================
// lookahead over the window of rows [carry ctx-1 | chunk J][N][H]
// ============================================================================================================
// ROWS: x and y hold the N rows that run the recurrent stack this feed; carry / next are the pool's two buffers [ctx-1][S][H]
template <typename T, bool ROWS>
__global__ void __launch_bounds__(256) k_stream_lookahead(const T* __restrict__ x, const T* __restrict__ carry, T* __restrict__ next,
                                                           const float* __restrict__ w, const int* __restrict__ len,
                                                           T* __restrict__ y, int N, int H, int ctx, int Jin, int off, int J,
                                                           const ds2_stream_row* __restrict__ rows, int S) {
  constexpr int V = Vec16<T>::N;
  const int hv = H / V, K = ctx - 1;
  const long nout = (long)J * N * hv, total = nout + (long)K * N * hv;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    const bool is_out = e < nout;
    const long q = is_out ? e : e - nout;
    const int h0 = (int)(q % hv) * V;
    const long rest = q / hv;
    const int n = (int)(rest % N), t = (int)(rest / N);
    int ln, nlive = J, cs = N, cn = n;                     // cs, cn: the carry's row stride and this stream's row in it
    bool fresh = false;
    const T* cr = carry;
    T* nx = next;
    if constexpr (ROWS) {
      const ds2_stream_row R = rows[n];
      ln = min(max(R.cnt2, 0), Jin);
      off = R.off3;
      nlive = R.cnt3;
      cs = S;
      cn = R.slot;
      fresh = (R.fresh & 4) != 0;
      if (R.cur & 4) {
        cr = next;
        nx = const_cast<T*>(carry);
      }
    } else {
      ln = len ? min(max(len[n], 0), Jin) : Jin;
    }
    if (!is_out) {                                         // next[t] = V[ln + t], t < K
      const int p = ln + t;
      const T* src = p < K ? cr + ((long)p * cs + cn) * H + h0 : x + ((long)(p - K) * N + n) * H + h0;
      uint4 val = *reinterpret_cast<const uint4*>(src);
      if (ROWS && fresh && p < K) val = make_uint4(0u, 0u, 0u, 0u);
      *reinterpret_cast<uint4*>(nx + ((long)t * cs + cn) * H + h0) = val;
      continue;
    }
    float acc[V];
#pragma unroll
    for (int i = 0; i < V; ++i) acc[i] = 0.f;
    for (int k = (ROWS && t >= nlive) ? ctx : 0; k < ctx; ++k) {      // ROWS: rows t >= cnt3 are written as zeros
      const int p = off + t + k;
      if (p >= K + ln) break;                              // everything beyond the chunk is zero
      if (ROWS && fresh && p < K) continue;                // fmaf(w, 0, acc) == acc
      float xv[V];
      Vec16<T>::load(p < K ? cr + ((long)p * cs + cn) * H + h0 : x + ((long)(p - K) * N + n) * H + h0, xv);
#pragma unroll
      for (int i = 0; i < V; ++i) acc[i] = fmaf(w[(long)(h0 + i) * ctx + k], xv[i], acc[i]);
    }
#pragma unroll
    for (int i = 0; i < V; ++i) acc[i] = fminf(fmaxf(acc[i], 0.f), 20.f);
    Vec16<T>::store(y + ((long)t * N + n) * H + h0, acc);
  }
}

inline bool conv_geometry(int f0, int& f1, int& f2) {
  f1 = (f0 + 2 * 20 - K1F) / 2 + 1;
  f2 = (f1 + 2 * 10 - K2F) / 2 + 1;
  return f0 >= 1 && f1 >= 1 && f2 >= 1;
}

inline long align256(long b) { return (b + 255) / 256 * 256; }

template <typename T, bool ROWS>
int stream_conv2_launch(const StreamConv2Args& a, hipStream_t st) {
  static bool attr[DS2_MAX_DEVICES];
  if (ds2_first_use_on_device(attr))
    (void)hipFuncSetAttribute((const void*)k_stream_conv2<T, ROWS>, hipFuncAttributeMaxDynamicSharedMemorySize, CT_SMEM);
  const int ntiles = ds2_cdiv(a.J, CT_TB);
  dim3 grid(ntiles + 1, ds2_cdiv(a.F2, CT_UB), a.N);
  hipLaunchKernelGGL((k_stream_conv2<T, ROWS>), grid, dim3(256), CT_SMEM, st, a, ntiles);
  DS2_CHECK_LAUNCH();
  return 0;
}

}  // namespace

extern "C" {

int ds2_stream_plan(long frames, int chunk, int ctx, int final_, int* out) {
  DS2_REQUIRE(out != nullptr && frames >= 0 && chunk >= 0 && ctx >= 1 && frames + chunk < (1L << 30), DS2_ERR_ARG);
  auto ends = [&](long G, bool fin, long* e) {
    if (fin) {
      e[0] = e[1] = e[2] = G > 0 ? (G - 1) / 2 + 1 : 0;
    } else {
      e[0] = G < 6 ? 0 : (G - 6) / 2 + 1;
      e[1] = e[0] > 5 ? e[0] - 5 : 0;
      e[2] = e[1] > ctx - 1 ? e[1] - (ctx - 1) : 0;
    }
  };
  long o[3], e[3];
  ends(frames, false, o);
  ends(frames + chunk, final_ != 0, e);
  for (int i = 0; i < 3; ++i) {
    out[2 * i] = (int)o[i];
    out[2 * i + 1] = (int)e[i];
  }
  out[6] = (int)(2 * o[0] + 5 - frames);            // window position of the first input frame conv1 frame J1_old reads
  out[7] = (int)(o[1] + 5 - o[0]);                  // ... of the first conv1 activation conv2 frame J2_old reads
  out[8] = (int)(o[2] + (ctx - 1) - o[1]);          // ... of RNN row J3_old
  out[9] = SK;
  out[10] = SK;
  out[11] = ctx - 1;
  return 0;
}

long ds2_stream_state_bytes(int dtype, int N, int F0_, int H, int ctx) {
  int f1, f2;
  if ((dtype != DS2_F32 && dtype != DS2_BF16) || N <= 0 || H <= 0 || ctx < 1 || !conv_geometry(F0_, f1, f2)) return 0;
  const long esz = dtype == DS2_F32 ? 4 : 2;
  return 2 * (align256((long)N * F0_ * SK * 4) + align256((long)N * f1 * SK * CH * esz) + align256((long)(ctx - 1) * N * H * esz));
}

int ds2_stream_conv1(int dtype, const float* x, const float* carry, float* next, const float* w1k, const float* b1,
                     const float* scale, const float* shift, const int* len, const int* live, void* y, int N, int F0_, int Tc,
                     int off, int J, ds2_stream_t st_) {
  hipStream_t st = (hipStream_t)st_;
  DS2_REQUIRE(dtype == DS2_F32 || dtype == DS2_BF16, DS2_ERR_DTYPE);
  int f1, f2;
  DS2_REQUIRE(N > 0 && N <= 65535 && Tc >= 0 && J >= 0 && off >= 0 && conv_geometry(F0_, f1, f2), DS2_ERR_ARG);
  DS2_REQUIRE(carry && next && carry != next && w1k && b1 && scale && shift && (x || Tc == 0) && (y || J == 0), DS2_ERR_ARG);
  const int ntiles = ds2_cdiv(J, C1_TB);
  dim3 grid(ntiles + 1, ds2_cdiv(f1, C1_FB), N);
  if (dtype == DS2_F32)
    hipLaunchKernelGGL((k_stream_conv1<float, false>), grid, dim3(256), 0, st, x, carry, next, w1k, b1, scale, shift, len, live, (float*)y,
                       N, Tc, off, J, F0_, f1, ntiles, nullptr);
  else
    hipLaunchKernelGGL((k_stream_conv1<bf16_t, false>), grid, dim3(256), 0, st, x, carry, next, w1k, b1, scale, shift, len, live,
                       (bf16_t*)y, N, Tc, off, J, F0_, f1, ntiles, nullptr);
  DS2_CHECK_LAUNCH();
  return 0;
}

int ds2_stream_conv2(int dtype, const void* a1, const void* carry, void* next, const void* w2t, const float* b2, const float* scale,
                     const float* shift, const int* len, const int* live, void* x0, int N, int F0_, int Jin, int off, int J,
                     int rld, ds2_stream_t st_) {
  hipStream_t st = (hipStream_t)st_;
  DS2_REQUIRE(dtype == DS2_F32 || dtype == DS2_BF16, DS2_ERR_DTYPE);
  int f1, f2;
  DS2_REQUIRE(N > 0 && N <= 65535 && Jin >= 0 && J >= 0 && off >= 0 && conv_geometry(F0_, f1, f2), DS2_ERR_ARG);
  DS2_REQUIRE(rld >= f2 * CH && rld % 16 == 0 && (long)J * N * rld < (1L << 31), DS2_ERR_ARG);
  DS2_REQUIRE(carry && next && carry != next && w2t && b2 && scale && shift && (a1 || Jin == 0) && (x0 || J == 0), DS2_ERR_ARG);
  StreamConv2Args a{a1, carry, next, w2t, b2, scale, shift, len, live, x0, N, Jin, off, J, f1, f2, rld, nullptr, N};
  return dtype == DS2_F32 ? stream_conv2_launch<float, false>(a, st) : stream_conv2_launch<bf16_t, false>(a, st);
}

int ds2_stream_lookahead(int dtype, const void* x, const void* carry, void* next, const float* w, const int* len, void* y, int N,
                         int H, int ctx, int Jin, int off, int J, ds2_stream_t st_) {
  hipStream_t st = (hipStream_t)st_;
  DS2_REQUIRE(dtype == DS2_F32 || dtype == DS2_BF16, DS2_ERR_DTYPE);
  const int V = dtype == DS2_F32 ? 4 : 8;
  DS2_REQUIRE(N > 0 && H > 0 && H % V == 0 && ctx >= 1 && Jin >= 0 && J >= 0 && off >= 0, DS2_ERR_ARG);
  DS2_REQUIRE(w && (x || Jin == 0) && (y || J == 0) && (ctx == 1 || (carry && next && carry != next)), DS2_ERR_ARG);
  const long total = ((long)J + ctx - 1) * N * (H / V);
  if (total == 0) return 0;
  const int grid = (int)(ds2_cdiv(total, 256) < 4096 ? ds2_cdiv(total, 256) : 4096);
  if (dtype == DS2_F32)
    hipLaunchKernelGGL((k_stream_lookahead<float, false>), dim3(grid), dim3(256), 0, st, (const float*)x, (const float*)carry,
                       (float*)next, w, len, (float*)y, N, H, ctx, Jin, off, J, nullptr, N);
  else
    hipLaunchKernelGGL((k_stream_lookahead<bf16_t, false>), dim3(grid), dim3(256), 0, st, (const bf16_t*)x, (const bf16_t*)carry,
                       (bf16_t*)next, w, len, (bf16_t*)y, N, H, ctx, Jin, off, J, nullptr, N);
  DS2_CHECK_LAUNCH();
  return 0;
}

// ---- the row-table entries: carry0 / carry1 are the two buffers of a stage's carries over the pool's S slots ----------------
int ds2_stream_conv1_rows(int dtype, const float* x, float* carry0, float* carry1, const ds2_stream_row* rows, const float* w1k,
                          const float* b1, const float* scale, const float* shift, void* y, int n_rows, int F0_, int Tc, int J,
                          ds2_stream_t st_) {
  hipStream_t st = (hipStream_t)st_;
  DS2_REQUIRE(dtype == DS2_F32 || dtype == DS2_BF16, DS2_ERR_DTYPE);
  int f1, f2;
  DS2_REQUIRE(n_rows > 0 && n_rows <= 65535 && Tc >= 0 && J >= 0 && conv_geometry(F0_, f1, f2), DS2_ERR_ARG);
  DS2_REQUIRE(rows && carry0 && carry1 && carry0 != carry1 && w1k && b1 && scale && shift && (x || Tc == 0) && (y || J == 0), DS2_ERR_ARG);
  const int ntiles = ds2_cdiv(J, C1_TB);
  dim3 grid(ntiles + 1, ds2_cdiv(f1, C1_FB), n_rows);
  if (dtype == DS2_F32)
    hipLaunchKernelGGL((k_stream_conv1<float, true>), grid, dim3(256), 0, st, x, carry0, carry1, w1k, b1, scale, shift, nullptr, nullptr,
                       (float*)y, n_rows, Tc, 0, J, F0_, f1, ntiles, rows);
  else
    hipLaunchKernelGGL((k_stream_conv1<bf16_t, true>), grid, dim3(256), 0, st, x, carry0, carry1, w1k, b1, scale, shift, nullptr, nullptr,
                       (bf16_t*)y, n_rows, Tc, 0, J, F0_, f1, ntiles, rows);
  DS2_CHECK_LAUNCH();
  return 0;
}

int ds2_stream_conv2_rows(int dtype, const void* a1, void* carry0, void* carry1, const ds2_stream_row* rows, const void* w2t,
                          const float* b2, const float* scale, const float* shift, void* x0, int n_rows, int n_rnn, int F0_, int Jin,
                          int J, int rld, ds2_stream_t st_) {
  hipStream_t st = (hipStream_t)st_;
  DS2_REQUIRE(dtype == DS2_F32 || dtype == DS2_BF16, DS2_ERR_DTYPE);
  int f1, f2;
  DS2_REQUIRE(n_rows > 0 && n_rows <= 65535 && n_rnn >= 0 && n_rnn <= n_rows && Jin >= 0 && J >= 0 && conv_geometry(F0_, f1, f2),
              DS2_ERR_ARG);
  DS2_REQUIRE(rld >= f2 * CH && rld % 16 == 0 && (long)J * n_rnn * rld < (1L << 31) && (J == 0) == (n_rnn == 0), DS2_ERR_ARG);
  DS2_REQUIRE(rows && carry0 && carry1 && carry0 != carry1 && w2t && b2 && scale && shift && (a1 || Jin == 0) && (x0 || J == 0),
              DS2_ERR_ARG);
  StreamConv2Args a{a1, carry0, carry1, w2t, b2, scale, shift, nullptr, nullptr, x0, n_rows, Jin, 0, J, f1, f2, rld, rows, n_rnn};
  return dtype == DS2_F32 ? stream_conv2_launch<float, true>(a, st) : stream_conv2_launch<bf16_t, true>(a, st);
}

int ds2_stream_lookahead_rows(int dtype, const void* x, void* carry0, void* carry1, const ds2_stream_row* rows, const float* w, void* y,
                              int n_rnn, int S, int H, int ctx, int Jin, int J, ds2_stream_t st_) {
  hipStream_t st = (hipStream_t)st_;
  DS2_REQUIRE(dtype == DS2_F32 || dtype == DS2_BF16, DS2_ERR_DTYPE);
  const int V = dtype == DS2_F32 ? 4 : 8;
  DS2_REQUIRE(n_rnn > 0 && S >= n_rnn && H > 0 && H % V == 0 && ctx >= 1 && Jin >= 0 && J >= 0, DS2_ERR_ARG);
  DS2_REQUIRE(rows && w && (x || Jin == 0) && (y || J == 0) && (ctx == 1 || (carry0 && carry1 && carry0 != carry1)), DS2_ERR_ARG);
  const long total = ((long)J + ctx - 1) * n_rnn * (H / V);
  if (total == 0) return 0;
  const int grid = (int)(ds2_cdiv(total, 256) < 4096 ? ds2_cdiv(total, 256) : 4096);
  if (dtype == DS2_F32)
    hipLaunchKernelGGL((k_stream_lookahead<float, true>), dim3(grid), dim3(256), 0, st, (const float*)x, (const float*)carry0,
                       (float*)carry1, w, nullptr, (float*)y, n_rnn, H, ctx, Jin, 0, J, rows, S);
  else
    hipLaunchKernelGGL((k_stream_lookahead<bf16_t, true>), dim3(grid), dim3(256), 0, st, (const bf16_t*)x, (const bf16_t*)carry0,
                       (bf16_t*)carry1, w, nullptr, (bf16_t*)y, n_rnn, H, ctx, Jin, 0, J, rows, S);
  DS2_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
