// CTC forced alignment: the Viterbi path of a KNOWN transcript through the network's outputs, with per-label frame spans.
//
// The lattice of ds2_ctc.hip with max in place of logsumexp, plus a trace-back.  For a target of L labels the extended sequence is
// ext[2i] = blank, ext[2i + 1] = target[i] (S = 2L + 1 states) and
//   v[0][0] = lp[0][blank], v[0][1] = lp[0][ext[1]], every other state -inf
//   v[t][s] = lp[t][ext[s]] + max(v[t-1][s], v[t-1][s-1], v[t-1][s-2])      (s-2 only for an odd s with ext[s] != ext[s-2])
// in fp32, unreachable states exactly -inf.  TIE RULE (part of the contract): among equal predecessors s, then s-1, then s-2; at the
// end an equal value goes to state 2L rather than 2L - 1.  The chosen path is therefore, among the best paths, the one whose state
// sequence read from the LAST frame backwards is lexicographically largest.
//
// Launches on the caller's stream:
//   k_align_lognorm   (mode 0 only) the log-normaliser of every valid frame, lz = max + log sum exp(x - max), with the summation
//                     order of ds2_ctc.hip's log-softmax pass (one thread per frame up to 256 classes, one wave per frame beyond), so
//                     that x[c] - lz is bit for bit the log-probability the loss kernel sees.  Only a target's own classes are ever
//                     needed, so no log-probability rows are stored: 4 bytes per frame instead of 4 C.
//   k_ctc_align       one workgroup of 256 threads per clip, thread j owns the states j, j + 256, ...  (NS per thread, a template
//                     parameter chosen from max_target_len).  The two live rows of v are in LDS; one LDS-only barrier per frame.  The
//                     emission terms do not depend on the recursion: every thread gathers its states' scores of K frames from global
//                     memory one chunk of K frames ahead.  Back-pointers (0, 1, 2), one byte per (t, s), go to the workspace.
//                     Then the SAME workgroup traces back: the walk is serial, but a walk over 64 frames can only visit the 127 states
//                     below its starting state, so the workgroup loads that [64][128] window of back-pointers into LDS with all its
//                     threads and thread 0 walks in LDS -- T'/64 rounds of global latency instead of T' dependent loads.  Last, one
//                     thread per label run sums the label's log-probabilities in increasing frame order.
// Every loop bound that encloses a barrier comes from sizes[n] and target_lengths[n] (uniform over the workgroup); no atomics, no
// other workgroup is waited for.  Results are the same bits on every launch.
#include <math.h>

#include "ds2_common.h"

namespace {

constexpr int AL_THREADS = 256;           // workgroup of k_ctc_align (tests/test_gpu_ctc_align.py names the same number)
constexpr int AL_MAX_TARGET_LEN = 2047;   // S = 4095 states: 16 per thread, 48 KB of LDS rows (+ the 8 KB trace-back tile)
constexpr int TB_FRAMES = 64;             // frames per trace-back round
constexpr int TB_WIDTH = 2 * TB_FRAMES;   // states a walk over TB_FRAMES frames can reach (2 per frame), rounded up

// workgroup barrier that orders LDS traffic only: the back-pointer stores and the prefetch loads stay in flight across it
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// mode 0: logits (lz = the frame's log-normaliser), 1: probabilities (logf(0) = -inf), 2: log-probabilities as they are
__device__ __forceinline__ float to_logp(float x, float lz, int mode) { return mode == 0 ? x - lz : mode == 1 ? logf(x) : x; }

// row stride of the back-pointer bytes and of the LDS rows: the 2 max_target_len + 1 states, rounded up to 4
__host__ __device__ inline int align_row_stride(int max_target_len) { return (2 * max_target_len + 4) & ~3; }

__global__ void __launch_bounds__(256) k_align_lognorm(const float* __restrict__ x, long stride_n, long stride_t,
                                                       const int* __restrict__ sizes, int Tp, int N, int C, float* __restrict__ lz) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;     // frame n*Tp + t
  if (i >= (long)N * Tp) return;
  const int n = (int)(i / Tp), t = (int)(i % Tp);
  if (sizes && t >= sizes[n]) return;
  const float* r = x + n * stride_n + t * stride_t;
  float m = -INFINITY;
  for (int c = 0; c < C; ++c) m = fmaxf(m, r[c]);
  float sum = 0.f;
  for (int c = 0; c < C; ++c) sum += expf(r[c] - m);
  lz[i] = m + logf(sum);
}

// more than 256 classes: one wave per frame, as ds2_ctc.hip's k_ctc_logsoftmax_big
__global__ void __launch_bounds__(256) k_align_lognorm_big(const float* __restrict__ x, long stride_n, long stride_t,
                                                           const int* __restrict__ sizes, int Tp, int N, int C, float* __restrict__ lz) {
  const long i = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (i >= (long)N * Tp) return;
  const int n = (int)(i / Tp), t = (int)(i % Tp);
  if (sizes && t >= sizes[n]) return;                      // wave-uniform
  const float* r = x + n * stride_n + t * stride_t;
  float m = -INFINITY;
  for (int c = lane; c < C; c += 64) m = fmaxf(m, r[c]);
  m = wave_max(m);
  float sum = 0.f;
  for (int c = lane; c < C; c += 64) sum += expf(r[c] - m);
  sum = wave_sum(sum);
  if (lane == 0) lz[i] = m + logf(sum);
}

// NS: states per thread (S <= NS * AL_THREADS); K: frames whose emission terms are gathered together, one chunk ahead
template <int NS, int K>
__global__ void __launch_bounds__(AL_THREADS) k_ctc_align(const float* __restrict__ x, long stride_n, long stride_t, int Tp, int C, int mode,
                                                          const int* __restrict__ sizes, const int* __restrict__ targets,
                                                          const int* __restrict__ toff, const int* __restrict__ tlen, int max_target_len,
                                                          int blank, const float* __restrict__ ws_lz, unsigned char* __restrict__ ws_bp,
                                                          int* __restrict__ frame_state, int* __restrict__ tok_start,
                                                          int* __restrict__ tok_end, float* __restrict__ tok_logp,
                                                          float* __restrict__ score) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int SS = align_row_stride(max_target_len);
  float* prev = reinterpret_cast<float*>(smem);            // the two live rows of v                     [SS] each
  float* cur = prev + SS;
  int* ext = reinterpret_cast<int*>(cur + SS);             // extended label sequence                   [SS]
  __shared__ unsigned char tile[TB_FRAMES][TB_WIDTH];      // back-pointer window of one trace-back round
  __shared__ int sh_state;
  __shared__ float sh_score;
  const int tid = threadIdx.x, n = blockIdx.x;
  int Ti = sizes ? sizes[n] : Tp;
  Ti = Ti < 0 ? 0 : Ti > Tp ? Tp : Ti;
  const int L = tlen[n];
  const bool bad_len = L < 0 || L > max_target_len;        // beyond what the caller sized LDS and workspace for: no lattice
  const int S = 2 * L + 1;
  int* fs = frame_state + (long)n * Tp;
  const int* tg = targets + toff[n];
  int* ts = tok_start + toff[n];
  int* te = tok_end + toff[n];
  float* tl = tok_logp + toff[n];
  // no path: every output of the clip says so (a clip with a target length outside [0, max_target_len] cannot be trusted to own
  // tok entries: only its score and frames are written)
  auto infeasible = [&]() {
    for (int t = tid; t < Tp; t += AL_THREADS) fs[t] = -1;
    if (!bad_len)
      for (int i = tid; i < L; i += AL_THREADS) {
        ts[i] = -1;
        te[i] = -1;
        tl[i] = 0.f;
      }
    if (tid == 0) score[n] = -INFINITY;
  };
  if (Ti == 0 || bad_len) {                                // uniform
    infeasible();
    return;
  }
  for (int s = tid; s < S; s += AL_THREADS) ext[s] = (s & 1) ? tg[s >> 1] : blank;
  __syncthreads();

  // ---- forward pass ---------------------------------------------------------------------------------------------------------
  // per-thread state tables.  Masks are additive: 0 = allowed, -inf = not (x + 0.f is exact, -inf + -inf = -inf).  A label outside
  // [0, C) has no emission: its states stay -inf and nothing is read for it.
  const float* xb = x + n * stride_n;
  const float* lzr = ws_lz + (long)n * Tp;
  unsigned char* bp = ws_bp + (long)n * Tp * SS;
  int st_c[NS];
  float st_m2[NS], st_mc[NS];
#pragma unroll
  for (int q = 0; q < NS; ++q) {
    const int s = tid + q * AL_THREADS;
    const int sc = s < S ? s : S - 1;
    const int e = ext[sc];
    const bool cok = e >= 0 && e < C;
    st_c[q] = cok ? e : 0;
    st_mc[q] = cok ? 0.f : -INFINITY;
    st_m2[q] = (sc >= 2 && (sc & 1) && e != ext[sc >= 2 ? sc - 2 : 0]) ? 0.f : -INFINITY;
  }
  float pe[K][NS], pz[K], nx[K][NS], nz[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int t = k < Ti ? k : Ti - 1;
    pz[k] = mode == 0 ? lzr[t] : 0.f;
#pragma unroll
    for (int q = 0; q < NS; ++q) pe[k][q] = xb[t * stride_t + st_c[q]];
  }
  for (int t0 = 0; t0 < Ti; t0 += K) {
#pragma unroll
    for (int k = 0; k < K; ++k) {
      int t = t0 + K + k;
      if (t > Ti - 1) t = Ti - 1;
      nz[k] = mode == 0 ? lzr[t] : 0.f;
#pragma unroll
      for (int q = 0; q < NS; ++q) nx[k][q] = xb[t * stride_t + st_c[q]];
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int t = t0 + k;
      if (t < Ti) {                                        // uniform
#pragma unroll
        for (int q = 0; q < NS; ++q) {
          const int s = tid + q * AL_THREADS;
          if (s < S) {
            const float a0 = prev[s];
            const float a1 = s >= 1 ? prev[s - 1] : -INFINITY;
            const float a2 = prev[s >= 2 ? s - 2 : 0] + st_m2[q];
            float best = a0;
            int b = 0;
            if (a1 > best) {
              best = a1;
              b = 1;
            }
            if (a2 > best) {
              best = a2;
              b = 2;
            }
            if (t == 0) {                                  // v[0]: the first blank and the first label
              best = s <= 1 ? 0.f : -INFINITY;
              b = 0;
            }
            cur[s] = best + (to_logp(pe[k][q], pz[k], mode) + st_mc[q]);
            bp[(long)t * SS + s] = (unsigned char)b;
          }
        }
        lds_barrier();
        float* tmp = prev;
        prev = cur;
        cur = tmp;
      }
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
      pz[k] = nz[k];
#pragma unroll
      for (int q = 0; q < NS; ++q) pe[k][q] = nx[k][q];
    }
  }
  // `prev` holds v[Ti - 1]
  if (tid == 0) {
    const float vb = prev[S - 1];
    const float vl = S > 1 ? prev[S - 2] : -INFINITY;
    const bool label_end = vl > vb;                        // an equal value goes to the final blank
    sh_score = label_end ? vl : vb;
    sh_state = label_end ? S - 2 : S - 1;
  }
  __syncthreads();                                         // also: every back-pointer store of the workgroup has landed
  const float best = sh_score;
  if (best == -INFINITY) {                                 // uniform
    infeasible();
    return;
  }
#ifndef DS2_ALIGN_SKIP_TRACEBACK     // A/B build of tools/time_ctc_align.py only (the forward pass alone; no outputs for feasible clips)
  // ---- trace-back -----------------------------------------------------------------------------------------------------------
  if (tid == 0) score[n] = best;
  for (int t = Ti + tid; t < Tp; t += AL_THREADS) fs[t] = -1;
  int s_hi = sh_state;
  for (int t_hi = Ti - 1; t_hi >= 1; t_hi -= TB_FRAMES) {  // uniform; frames t_hi .. t_hi - cnt + 1 (frame 0 has no predecessor)
    const int cnt = t_hi < TB_FRAMES ? t_hi : TB_FRAMES;
    // after k steps the walk is at most 2k states below s_hi: tile[k][j] = bp[t_hi - k][s_hi - j], 0 <= j <= 2k
    for (int e = tid; e < cnt * TB_WIDTH; e += AL_THREADS) {
      const int k = e / TB_WIDTH, j = e % TB_WIDTH;
      if (j <= 2 * k && s_hi - j >= 0) tile[k][j] = bp[(long)(t_hi - k) * SS + (s_hi - j)];
    }
    __syncthreads();
    if (tid == 0) {
      int s = s_hi;
      for (int k = 0; k < cnt; ++k) {
        fs[t_hi - k] = s;
        s -= tile[k][s_hi - s];
      }
      sh_state = s;
    }
    __syncthreads();
    s_hi = sh_state;
  }
  if (tid == 0) fs[0] = s_hi;
  __syncthreads();                                         // the clip's frame states are visible to the whole workgroup
  // ---- label spans: the thread of a label run's first frame walks the run ----------------------------------------------------
  for (int t = tid; t < Ti; t += AL_THREADS) {
    const int s = fs[t];
    if ((s & 1) && (t == 0 || fs[t - 1] != s)) {
      const int e = ext[s];
      float sum = 0.f;
      int t2 = t;
      do {
        sum += to_logp(xb[t2 * stride_t + e], mode == 0 ? lzr[t2] : 0.f, mode);
        ++t2;
      } while (t2 < Ti && fs[t2] == s);
      ts[s >> 1] = t;
      te[s >> 1] = t2 - 1;
      tl[s >> 1] = sum;
    }
  }
#endif
}

}  // namespace

extern "C" {

long ds2_ctc_align_ws_bytes(int Tp, int N, int max_target_len) {
  if (Tp < 1 || N < 1 || max_target_len < 0 || max_target_len > AL_MAX_TARGET_LEN) return -1;
  return (long)N * Tp * 4 + (long)N * Tp * align_row_stride(max_target_len);     // log-normalisers, then the back-pointer bytes
}

int ds2_ctc_align(const float* x, long stride_n, long stride_t, int N, int Tp, int C, int mode, const int* sizes, const int* targets,
                  const int* target_offsets, const int* target_lengths, int max_target_len, int blank, int* frame_state, int* tok_start,
                  int* tok_end, float* tok_logp, float* score, void* ws, ds2_stream_t st_) {
  hipStream_t st = (hipStream_t)st_;
  DS2_REQUIRE(N > 0 && Tp > 0 && C > 0 && blank >= 0 && blank < C && mode >= 0 && mode <= 2, DS2_ERR_ARG);
  DS2_REQUIRE(max_target_len >= 0 && max_target_len <= AL_MAX_TARGET_LEN, DS2_ERR_ARG);
  DS2_REQUIRE(x && targets && target_offsets && target_lengths && frame_state && tok_start && tok_end && tok_logp && score && ws,
              DS2_ERR_ARG);
  float* ws_lz = static_cast<float*>(ws);
  unsigned char* ws_bp = reinterpret_cast<unsigned char*>(ws_lz + (long)N * Tp);
  if (mode == 0) {
    if (C <= 256)
      hipLaunchKernelGGL(k_align_lognorm, dim3(ds2_cdiv((long)N * Tp, 256)), dim3(256), 0, st, x, stride_n, stride_t, sizes, Tp, N, C, ws_lz);
    else
      hipLaunchKernelGGL(k_align_lognorm_big, dim3(ds2_cdiv((long)N * Tp, 4)), dim3(256), 0, st, x, stride_n, stride_t, sizes, Tp, N, C,
                         ws_lz);
    DS2_CHECK_LAUNCH();
  }
  const int S = 2 * max_target_len + 1;
  const size_t shm = (size_t)align_row_stride(max_target_len) * 12;     // <= 48 KB at the cap, 56 KB with the static tile: under 64 KB, no attribute
#define DS2_ALIGN_LAUNCH(NS, K)                                                                                                       \
  hipLaunchKernelGGL((k_ctc_align<NS, K>), dim3(N), dim3(AL_THREADS), shm, st, x, stride_n, stride_t, Tp, C, mode, sizes, targets,    \
                     target_offsets, target_lengths, max_target_len, blank, ws_lz, ws_bp, frame_state, tok_start, tok_end, tok_logp,  \
                     score)
  if (S <= AL_THREADS) DS2_ALIGN_LAUNCH(1, 8);
  else if (S <= 2 * AL_THREADS) DS2_ALIGN_LAUNCH(2, 8);
  else if (S <= 4 * AL_THREADS) DS2_ALIGN_LAUNCH(4, 8);
  else DS2_ALIGN_LAUNCH(16, 2);
#undef DS2_ALIGN_LAUNCH
  DS2_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
