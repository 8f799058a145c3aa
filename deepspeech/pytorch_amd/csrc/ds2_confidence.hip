// Word timings and confidence for hypotheses that a CTC decoder returned (include/ds2hip.h "confidence").
//
// Launches on the caller's stream:
//   k_conf_frames   one wave per valid frame (4 frames per workgroup).  Lane j reads classes j, j + 64, ... of the frame's row
//                   (coalesced) and the wave forms
//                     a_t  the first maximal class, by the greedy decoder's rule: x[0] wins when it is NaN, a NaN elsewhere never
//                          wins (lane-local first maximum, then a butterfly that prefers the larger value and, among equal values,
//                          the smaller class)
//                     lz   (logits only) m + log(sum exp(x - m)) in fp64, rounded once to fp32
//                     m_t  the frame value of the measure.  The sums over the classes (lz's, the entropies') are fp64 and run in ONE
//                          order at every C: lane j adds its classes in increasing order, then the 64 partial sums are combined by
//                          v += shfl_xor(v, o) for o = 32, 16, ..., 1 (k_align_lognorm_big's order).  Seams of this map: C = 64, 128, ...
//                   8 bytes per frame go out (12 for logits), whatever C is.
//   k_conf_hyp      one wave per hypothesis, grid (B, N).  Tokens in chunks of 64, one per lane: the token's span by the two walks
//                   over a_t (it recomputes its left neighbour's forward end itself, so no token waits for another), its confidence
//                   over the span in increasing frame order (fp64, rounded once), word numbers by ballot + popcount of the "starts a
//                   word" flags carried across chunks.  Then one lane per word aggregates its tokens, then lane 0 the words.
//                   Every loop that encloses a barrier is bounded by the hypothesis' length or word count, the same for all 64 lanes
//                   (the workgroup IS the wave).  No atomics; every output element is written; same bits on every launch.
//   k_store_append / k_store_advance (ds2_frame_store_append)   a stream keeps its frames for this pass: chunk row j of stream n
//                   goes to row (count[n] + j) mod cap of the stream's store, the sizes and counts being read on the device; the
//                   second launch then adds sizes to count.
// Frame t of hypothesis row n is read at row (t0[n] + t) mod cap of x (one-shot calls: t0 = null, cap = Tp).
#include <math.h>

#include "ds2_common.h"

namespace {

constexpr int CF_MAX_CLASSES = 8192, CF_MAX_BEAMS = 256;
enum { M_LABEL_PROB = 0, M_MAX_PROB = 1, M_ENTROPY = 2, M_TSALLIS = 3, M_RENYI = 4 };
enum { AGG_MEAN = 0, AGG_MIN = 1, AGG_PROD = 2 };

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// p_t(c) as an fp32 number; kind 0: logits, 1: probabilities as given, 2: log-probabilities
__device__ __forceinline__ float conf_prob(float x, float lz, int kind) {
  return kind == 1 ? x : kind == 0 ? (float)exp((double)x - (double)lz) : (float)exp((double)x);
}

__device__ __forceinline__ int ring_row(const int* __restrict__ t0, int n, int t, int cap) {
  return t0 ? (int)(((long)t0[n] + t) % cap) : t;
}

__device__ __forceinline__ float clamp01(double v) { return (float)(v < 0.0 ? 0.0 : v > 1.0 ? 1.0 : v); }

__global__ void __launch_bounds__(256) k_conf_frames(const float* __restrict__ x, long stride_n, long stride_t, const int* __restrict__ sizes,
                                                     const int* __restrict__ t0, int cap, int N, int Tp, int C, int kind, int measure,
                                                     double alpha, int* __restrict__ fa, float* __restrict__ fm, float* __restrict__ flz) {
  const long i = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (i >= (long)N * Tp) return;                           // wave-uniform
  const int n = (int)(i / Tp), t = (int)(i % Tp);
  int Ti = sizes ? sizes[n] : Tp;
  Ti = Ti > Tp ? Tp : Ti;
  if (t >= Ti) return;                                     // wave-uniform
  const float* r = x + n * stride_n + (long)ring_row(t0, n, t, cap) * stride_t;
  // ---- a_t ----
  float kv = -INFINITY;                                    // a NaN counts as -inf: `v > best` is false for it
  int bc = 0x7fffffff;                                     // a lane without a class loses every tie
  for (int c = lane; c < C; c += 64) {
    float v = r[c];
    v = v != v ? -INFINITY : v;
    if (bc == 0x7fffffff || v > kv) {
      kv = v;
      bc = c;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(kv, o, 64);
    const int oc = __shfl_xor(bc, o, 64);
    if (ov > kv || (ov == kv && oc < bc)) {
      kv = ov;
      bc = oc;
    }
  }
  const float x0 = r[0];
  const int a = x0 != x0 ? 0 : bc;                         // ... except in class 0, where the greedy kernel's scan starts
  // ---- lz ----
  float lz = 0.f;
  if (kind == 0) {
    float m = -INFINITY;
    for (int c = lane; c < C; c += 64) m = fmaxf(m, r[c]);
    m = wave_max(m);
    double s = 0.0;
    for (int c = lane; c < C; c += 64) s += exp((double)r[c] - (double)m);
    s = wave_sum_f64(s);
    lz = (float)((double)m + log(s));
  }
  // ---- m_t ----
  float mt;
  if (measure <= M_MAX_PROB) {
    mt = conf_prob(r[a], lz, kind);
  } else {
    double s = 0.0;
    for (int c = lane; c < C; c += 64) {
      const double p = (double)conf_prob(r[c], lz, kind);
      if (measure == M_ENTROPY) s += p == 0.0 ? 0.0 : p * log(p);
      else s += pow(p, alpha);
    }
    s = wave_sum_f64(s);
    const double lnV = log((double)C);
    double v;
    if (measure == M_ENTROPY) v = 1.0 - (-s) / lnV;
    else if (measure == M_TSALLIS) v = 1.0 - ((1.0 - s) / (alpha - 1.0)) / ((1.0 - pow((double)C, 1.0 - alpha)) / (alpha - 1.0));
    else v = 1.0 - (log(s) / (1.0 - alpha)) / lnV;
    mt = clamp01(v);
  }
  if (lane == 0) {
    fa[i] = a;
    fm[i] = mt;
    if (kind == 0) flz[i] = lz;
  }
}

// mean / min / prod of values taken in order: fp64 accumulation, one rounding; min compares fp32 values (exact)
struct Agg {
  double acc;
  float mn;
  int cnt;
  __device__ __forceinline__ void init() {
    acc = 0.0;
    mn = 0.f;
    cnt = 0;
  }
  __device__ __forceinline__ void add(float v, int kind) {
    if (kind == AGG_MEAN) acc += (double)v;
    else if (kind == AGG_PROD) acc = cnt == 0 ? (double)v : acc * (double)v;
    else mn = (cnt == 0 || v < mn) ? v : mn;
    ++cnt;
  }
  __device__ __forceinline__ float get(int kind) const {
    if (cnt == 0) return NAN;
    return kind == AGG_MEAN ? (float)(acc / (double)cnt) : kind == AGG_PROD ? (float)acc : mn;
  }
};

// forward end of the token at frame o with label l; nxt: the next token's frame (Ti when there is none)
__device__ __forceinline__ int walk_fwd(const int* __restrict__ fa, int o, int l, int Ti, int nxt) {
  int e = o;
  const int lim = nxt < Ti ? nxt : Ti;
  while (e + 1 < lim && fa[e + 1] == l) ++e;
  return e;
}

__global__ void __launch_bounds__(64) k_conf_hyp(const float* __restrict__ x, long stride_n, long stride_t, const int* __restrict__ sizes,
                                                 const int* __restrict__ t0, int cap, int Tp, int C, int kind, int measure, int agg,
                                                 int wagg, int space, const int* __restrict__ tokens, const int* __restrict__ offsets,
                                                 const int* __restrict__ lens, int B, int ld, int lw, const int* __restrict__ fa_,
                                                 const float* __restrict__ fm_, const float* __restrict__ flz_,
                                                 int* __restrict__ tok_start, int* __restrict__ tok_end, float* __restrict__ tok_conf,
                                                 int* __restrict__ word_first, int* __restrict__ word_last, int* __restrict__ word_start,
                                                 int* __restrict__ word_end, float* __restrict__ word_conf, int* __restrict__ word_count,
                                                 float* __restrict__ utt_conf) {
  const int b = blockIdx.x, n = blockIdx.y, lane = threadIdx.x;
  const long h = (long)n * B + b;
  int Ti = sizes ? sizes[n] : Tp;
  Ti = Ti < 0 ? 0 : Ti > Tp ? Tp : Ti;
  const int* tok = tokens + h * ld;
  const int* off = offsets + h * ld;
  int* ts = tok_start + h * ld;
  int* te = tok_end + h * ld;
  float* tc = tok_conf + h * ld;
  int* wf = word_first + h * lw;
  int* wl = word_last + h * lw;
  int* ws = word_start + h * lw;
  int* we = word_end + h * lw;
  float* wc = word_conf + h * lw;
  const int* fa = fa_ + (long)n * Tp;
  const float* fm = fm_ + (long)n * Tp;
  const float* flz = flz_ + (long)n * Tp;
  const float* xb = x + n * stride_n;
  const int L = lens[h];
  // ---- an index that cannot be trusted: nothing of the hypothesis is used as one ----
  bool bad = L < 0 || L > ld;
  if (!bad) {
    int any = 0;
    for (int i = lane; i < L; i += 64) {
      const int l = tok[i], o = off[i];
      any |= (l < 0 || l >= C || o < 0 || o >= Ti) ? 1 : 0;
    }
    bad = __ballot(any) != 0ull;
  }
  const int Lv = bad ? 0 : L;                              // wave-uniform
  // ---- tokens ----
  int nwords = 0;
  for (int i0 = 0; i0 < Lv; i0 += 64) {                    // uniform
    const int i = i0 + lane;
    const bool live = i < Lv;
    int l = -1, s = -1, e = -1;
    bool starts = false, ends = false;
    if (live) {
      l = tok[i];
      const int o = off[i];
      e = walk_fwd(fa, o, l, Ti, i + 1 < Lv ? off[i + 1] : Ti);
      int floor_t = -1;                                    // the walk back stops above the previous token's forward end
      int lp = space;
      if (i > 0) {
        lp = tok[i - 1];
        floor_t = walk_fwd(fa, off[i - 1], lp, Ti, o);
      }
      s = o;
      while (s - 1 >= 0 && s - 1 > floor_t && fa[s - 1] == l) --s;
      Agg g;
      g.init();
      for (int t = s; t <= e; ++t) {
        float v;
        if (measure == M_LABEL_PROB)
          v = conf_prob(xb[(long)ring_row(t0, n, t, cap) * stride_t + l], kind == 0 ? flz[t] : 0.f, kind);
        else
          v = fm[t];
        g.add(v, agg);
      }
      ts[i] = s;
      te[i] = e;
      tc[i] = g.get(agg);
      const bool word_tok = l != space;
      starts = word_tok && (i == 0 || lp == space);
      ends = word_tok && (i + 1 == Lv || tok[i + 1] == space);
    }
    const unsigned long long ms = __ballot(starts);
    const int upto = nwords + __popcll(ms & ((2ull << lane) - 1ull));      // word starts at or before this token
    if (starts) {
      wf[upto - 1] = i;
      ws[upto - 1] = s;
    }
    if (ends) {
      wl[upto - 1] = i;
      we[upto - 1] = e;
    }
    nwords += __popcll(ms);
  }
  for (int i = Lv + lane; i < ld; i += 64) {
    ts[i] = -1;
    te[i] = -1;
    tc[i] = NAN;
  }
  __syncthreads();                                         // the wave's token and word-table stores are visible to all its lanes
  // ---- words: one lane each ----
  for (int w = lane; w < lw; w += 64) {
    if (w < nwords) {
      Agg g;
      g.init();
      const int last = wl[w];
      for (int i = wf[w]; i <= last; ++i) g.add(tc[i], wagg);
      wc[w] = g.get(wagg);
    } else {
      wf[w] = -1;
      wl[w] = -1;
      ws[w] = -1;
      we[w] = -1;
      wc[w] = NAN;
    }
  }
  __syncthreads();
  if (lane == 0) {
    Agg g;
    g.init();
    for (int w = 0; w < nwords; ++w) g.add(wc[w], wagg);
    utt_conf[h] = g.get(wagg);                             // NaN without words
    word_count[h] = nwords;
  }
}

// chunk row j of stream n -> store row (count[n] + j) mod cap; grid (ceil(Tc / 4), N), one wave per row
__global__ void __launch_bounds__(256) k_store_append(const float* __restrict__ x, long stride_n, long stride_t, int Tc, int C,
                                                      const int* __restrict__ sizes, const int* __restrict__ count,
                                                      float* __restrict__ store, int cap) {
  const int n = blockIdx.y, j = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  int sz = sizes ? sizes[n] : Tc;
  sz = sz > Tc ? Tc : sz;
  if (j >= sz) return;
  const float* r = x + n * stride_n + (long)j * stride_t;
  float* d = store + ((long)n * cap + (int)(((long)count[n] + j) % cap)) * C;
  for (int c = lane; c < C; c += 64) d[c] = r[c];
}

__global__ void __launch_bounds__(64) k_store_advance(int N, int Tc, const int* __restrict__ sizes, int* __restrict__ count) {
  const int n = blockIdx.x * 64 + threadIdx.x;
  if (n >= N) return;
  int sz = sizes ? sizes[n] : Tc;
  sz = sz < 0 ? 0 : sz > Tc ? Tc : sz;
  count[n] += sz;
}

}  // namespace

extern "C" {

long ds2_confidence_ws_bytes(int N, int Tp) {
  if (N < 1 || Tp < 1) return -1;
  return (long)N * Tp * 12;                                // a_t, m_t, lz
}

int ds2_confidence(const float* x, long stride_n, long stride_t, int N, int Tp, int C, int kind, const int* sizes, const int* t0,
                   int cap, const int* tokens, const int* offsets, const int* lens, int B, int ld, int lw, int blank, int space,
                   int measure, double alpha, int aggregate, int word_aggregate, int* tok_start, int* tok_end, float* tok_conf,
                   int* word_first, int* word_last, int* word_start, int* word_end, float* word_conf, int* word_count,
                   float* utt_conf, void* ws, ds2_stream_t st_) {
  hipStream_t st = (hipStream_t)st_;
  DS2_REQUIRE(N > 0 && N <= 65535 && Tp > 0 && C > 0 && C <= CF_MAX_CLASSES && B > 0 && B <= CF_MAX_BEAMS && ld > 0 && 2 * (long)lw >= ld, DS2_ERR_ARG);
  DS2_REQUIRE((long)N * Tp <= 0x7fffffffL, DS2_ERR_ARG);      // the frame kernel's grid and the [N][Tp] workspace index
  DS2_REQUIRE(blank >= 0 && blank < C && space >= 0 && kind >= 0 && kind <= 2 && cap >= Tp, DS2_ERR_ARG);
  DS2_REQUIRE(measure >= M_LABEL_PROB && measure <= M_RENYI && aggregate >= 0 && aggregate <= 2 && word_aggregate >= 0 &&
                  word_aggregate <= 2,
              DS2_ERR_ARG);
  if (measure >= M_ENTROPY) DS2_REQUIRE(C >= 2, DS2_ERR_ARG);
  if (measure >= M_TSALLIS) DS2_REQUIRE(alpha > 0.0 && alpha != 1.0, DS2_ERR_ARG);
  DS2_REQUIRE(x && tokens && offsets && lens && tok_start && tok_end && tok_conf && word_first && word_last && word_start && word_end &&
                  word_conf && word_count && utt_conf && ws,
              DS2_ERR_ARG);
  int* fa = static_cast<int*>(ws);
  float* fm = reinterpret_cast<float*>(fa + (long)N * Tp);
  float* flz = fm + (long)N * Tp;
  hipLaunchKernelGGL(k_conf_frames, dim3(ds2_cdiv((long)N * Tp, 4)), dim3(256), 0, st, x, stride_n, stride_t, sizes, t0, cap, N, Tp, C, kind,
                     measure, alpha, fa, fm, flz);
  DS2_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_conf_hyp, dim3(B, N), dim3(64), 0, st, x, stride_n, stride_t, sizes, t0, cap, Tp, C, kind, measure, aggregate,
                     word_aggregate, space, tokens, offsets, lens, B, ld, lw, fa, fm, flz, tok_start, tok_end, tok_conf, word_first,
                     word_last, word_start, word_end, word_conf, word_count, utt_conf);
  DS2_CHECK_LAUNCH();
  return 0;
}

int ds2_frame_store_append(const float* x, long stride_n, long stride_t, int N, int Tc, int C, const int* sizes, int* count, float* store,
                           int cap, ds2_stream_t st_) {
  hipStream_t st = (hipStream_t)st_;
  DS2_REQUIRE(N > 0 && N <= 65535 && Tc > 0 && C > 0 && C <= CF_MAX_CLASSES && cap >= Tc && x && count && store, DS2_ERR_ARG);
  hipLaunchKernelGGL(k_store_append, dim3(ds2_cdiv(Tc, 4), N), dim3(256), 0, st, x, stride_n, stride_t, Tc, C, sizes, count, store, cap);
  DS2_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_store_advance, dim3(ds2_cdiv(N, 64)), dim3(64), 0, st, N, Tc, sizes, count);
  DS2_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
