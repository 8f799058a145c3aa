// Keyword spotting on the CTC outputs (the rule is stated in include/ds2hip.h): the max-lattice of
// ds2_align.hip over a keyword's labels with a FREE start and a FREE end, scored against the greedy path, carried across feeds.
//
// Launches of one ds2_kws_feed on the caller's stream:
//   k_kws_framemax   max_c lp of every valid frame (4 bytes per frame, as k_align_lognorm); one thread per frame up to 256 classes,
//                    one wave per frame beyond.  For probabilities the maximum is taken first and logf once: logf is monotone.
//   k_kws_lattice    the host packs the keywords into waves of 64 lanes (no keyword straddles a wave); lane i of a keyword holds
//                    the label state y_i and the blank state after it, value and start frame each, in registers.  One wave walks
//                    its keywords of one stream through the feed's frames: per frame four DPP wave shifts (ds2_ctc.hip's) bring the
//                    previous lane's two values and two start frames, then compares and selects.  No LDS, no barrier.  A lane's label
//                    score, the blank score and the frame maximum are gathered KW_AHEAD frames ahead (k_ctc_align's scheme); the last
//                    two are the same address for the whole wave.  KW_WPB waves of one stream share a workgroup, so a row is fetched
//                    into the CU's cache once for all of them.  The lane of a keyword's last label owns the keyword's candidate,
//                    best and hit count and writes the hits of this feed to the keyword's list in the workspace.
//   k_kws_compact    one workgroup per stream: an exclusive scan of the keywords' hit counts, the hits moved to one list per stream
//                    in (keyword, time) order behind a header (hits, dropped, frames).
// No atomics, nothing waits for another workgroup, no value depends on a launch's timing: the same bits on every launch.
#include <math.h>

#include "ds2_common.h"

namespace {

constexpr int KW_WPB = 4;            // waves of one stream per workgroup
constexpr int KW_AHEAD = 8;          // frames whose scores are gathered together, one chunk ahead
constexpr int KW_LAT_WORDS = 4;      // per (stream, lane): label value, blank value, label start, blank start
constexpr int KW_KEY_WORDS = 8;      // per (stream, keyword): candidate score, start, end; best score, start, end; 2 reserved
constexpr int KW_HDR = 4;            // header of a stream's output row: hits, dropped, frames consumed, 0
constexpr int KW_HIT_WORDS = 4;      // a hit of the output row: keyword, start, end, score bits
constexpr int KW_FIRST = 1, KW_LAST = 2, KW_SKIP = 4;   // lane flags (tests/test_kws_host.py and keywords.pack name the same bits)
constexpr int KW_MAX_HITS = 4096;
constexpr int KW_MAX_STREAMS = 65535;                    // grid.y of the lattice pass

struct KwState {
  float* lat;     // [N][W][KW_LAT_WORDS][64]
  int* key;       // [N][K][KW_KEY_WORDS]
  int* frm;       // [N][W] frames consumed, one copy per wave: no wave reads what another writes
};

__host__ __device__ inline long kw_lat_words(int N, int W) { return (long)N * W * KW_LAT_WORDS * 64; }
__host__ __device__ inline long kw_key_words(int N, int K) { return (long)N * K * KW_KEY_WORDS; }

inline KwState kw_state(void* state, int N, int W, int K) {
  KwState s;
  s.lat = static_cast<float*>(state);
  s.key = reinterpret_cast<int*>(s.lat + kw_lat_words(N, W));
  s.frm = s.key + kw_key_words(N, K);
  return s;
}

inline long kw_ws_fmax_words(int N, int Tc) { return ((long)N * Tc + 3) & ~3l; }

// lane i <- lane i - 1 of the whole wave in one VALU instruction; lane 0 gets 0 and is always a keyword's first lane or unused
__device__ __forceinline__ float kw_below(float v) {
  return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x138 /* wave_shr:1 */, 0xf, 0xf, true));
}
__device__ __forceinline__ int kw_below(int v) { return __builtin_amdgcn_mov_dpp(v, 0x138 /* wave_shr:1 */, 0xf, 0xf, true); }

// mode 0: logits, 1: probabilities, 2: log-probabilities (ds2_ctc_align's numbering); logits need no normaliser here, it cancels
__device__ __forceinline__ float kw_lp(float x, int mode) { return mode == 1 ? logf(x) : x; }

__device__ __forceinline__ int kw_size(const int* sizes, int n, int Tc) {
  int s = sizes ? sizes[n] : Tc;
  return s < 0 ? 0 : (s > Tc ? Tc : s);
}

__global__ void __launch_bounds__(256) k_kws_framemax(const float* __restrict__ x, long stride_n, long stride_t,
                                                      const int* __restrict__ sizes, int Tc, int N, int C, int mode,
                                                      float* __restrict__ fmax) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;     // frame n * Tc + t
  if (i >= (long)N * Tc) return;
  const int n = (int)(i / Tc), t = (int)(i % Tc);
  if (t >= kw_size(sizes, n, Tc)) return;
  const float* r = x + n * stride_n + t * stride_t;
  float m = -INFINITY;
  for (int c = 0; c < C; ++c) m = fmaxf(m, r[c]);
  fmax[i] = kw_lp(m, mode);
}

__global__ void __launch_bounds__(256) k_kws_framemax_big(const float* __restrict__ x, long stride_n, long stride_t,
                                                          const int* __restrict__ sizes, int Tc, int N, int C, int mode,
                                                          float* __restrict__ fmax) {
  const long i = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (i >= (long)N * Tc) return;
  const int n = (int)(i / Tc), t = (int)(i % Tc);
  if (t >= kw_size(sizes, n, Tc)) return;                  // wave-uniform
  const float* r = x + n * stride_n + t * stride_t;
  float m = -INFINITY;
  for (int c = lane; c < C; c += 64) m = fmaxf(m, r[c]);
  m = wave_max(m);
  if (lane == 0) fmax[i] = kw_lp(m, mode);
}

__global__ void __launch_bounds__(KW_WPB * 64) k_kws_lattice(const float* __restrict__ x, long stride_n, long stride_t, int Tc, int C,
                                                             int mode, const int* __restrict__ sizes, int blank,
                                                             const int4* __restrict__ lanes, int W, int K, int hold, int max_hits,
                                                             const int* __restrict__ end_mask, int end_all, float* __restrict__ lat,
                                                             int* __restrict__ key, int* __restrict__ frm,
                                                             const float* __restrict__ fmax, int* __restrict__ hit_cnt,
                                                             int* __restrict__ hits) {
  const int lane = threadIdx.x & 63;
  const int w = blockIdx.x * KW_WPB + (threadIdx.x >> 6);
  const int n = blockIdx.y;
  if (w >= W) return;                                      // wave-uniform; the kernel has no barrier
  const int size = Tc > 0 ? kw_size(sizes, n, Tc) : 0;
  const bool ending = end_all != 0 || (end_mask && end_mask[n] != 0);
  const int4 meta = lanes[w * 64 + lane];
  const int label = meta.x, flags = meta.y, kw = meta.z;
  const float thr = __int_as_float(meta.w);
  const bool used = label >= 0 && label < C;               // a lane without a label keeps -inf and reads the blank column
  const bool first = (flags & KW_FIRST) != 0;
  const bool skip = (flags & KW_SKIP) != 0 && !first;
  const bool tail = (flags & KW_LAST) != 0;                // the keyword's last label: no blank state after it
  const bool owner = tail && used && kw >= 0 && kw < K;    // this lane owns keyword kw's candidate, best and hits
  const long nk = (long)n * K + (owner ? kw : 0);
  int* hl = hits + nk * max_hits * 3;
  if (size == 0 && !ending) {                              // the state is left bitwise as it is
    if (owner) hit_cnt[nk] = 0;
    return;
  }
  float* ls = lat + ((long)n * W + w) * (KW_LAT_WORDS * 64) + lane;
  float v_lab = ls[0], v_blk = ls[64];
  int b_lab = __float_as_int(ls[128]), b_blk = __float_as_int(ls[192]);
  int* ks = key + nk * KW_KEY_WORDS;
  float c_s = -INFINITY, m_s = -INFINITY;                  // the open candidate (c_e < 0: none) and the best so far
  int c_b = -1, c_e = -1, m_b = -1, m_e = -1;
  if (owner) {
    const int4 a = *reinterpret_cast<const int4*>(ks), b = *reinterpret_cast<const int4*>(ks + 4);
    c_s = __int_as_float(a.x), c_b = a.y, c_e = a.z;
    m_s = __int_as_float(a.w), m_b = b.x, m_e = b.y;
  }
  const int t_base = frm[(long)n * W + w];
  int cnt = 0;
  auto emit = [&]() {
    if (cnt < max_hits) {
      hl[cnt * 3] = c_b;
      hl[cnt * 3 + 1] = c_e;
      hl[cnt * 3 + 2] = __float_as_int(c_s);
    }
    ++cnt;
    c_s = -INFINITY;
    c_b = -1;
    c_e = -1;
  };
  if (size > 0) {
    const float* xb = x + n * stride_n;
    const float* fm = fmax + (long)n * Tc;
    const int col = used ? label : blank;
    float pe[KW_AHEAD], pb[KW_AHEAD], pm[KW_AHEAD], ne[KW_AHEAD], nb[KW_AHEAD], nm[KW_AHEAD];
#pragma unroll
    for (int k = 0; k < KW_AHEAD; ++k) {
      const int t = k < size ? k : size - 1;               // frames at and beyond size are never read
      pe[k] = xb[t * stride_t + col];
      pb[k] = xb[t * stride_t + blank];
      pm[k] = fm[t];
    }
    for (int t0 = 0; t0 < size; t0 += KW_AHEAD) {
#pragma unroll
      for (int k = 0; k < KW_AHEAD; ++k) {
        int t = t0 + KW_AHEAD + k;
        if (t > size - 1) t = size - 1;
        ne[k] = xb[t * stride_t + col];
        nb[k] = xb[t * stride_t + blank];
        nm[k] = fm[t];
      }
#pragma unroll
      for (int k = 0; k < KW_AHEAD; ++k) {
        const int t = t0 + k;
        if (t < size) {                                    // wave-uniform: every lane takes part in the shifts
          const int ta = t_base + t;
          const float r_lab = used ? kw_lp(pe[k], mode) - pm[k] : -INFINITY;
          const float r_blk = kw_lp(pb[k], mode) - pm[k];
          float a1 = kw_below(v_blk), a2 = kw_below(v_lab);
          int a1b = kw_below(b_blk), a2b = kw_below(b_lab);
          if (first) {                                     // state 0: the fresh start stands where s - 1 does
            a1 = 0.f;
            a1b = ta;
          }
          if (!skip) a2 = -INFINITY;
          float best = v_lab, best2 = v_blk;
          int bb = b_lab, bb2 = b_blk;
          if (a1 > best) {
            best = a1;
            bb = a1b;
          }
          if (a2 > best) {
            best = a2;
            bb = a2b;
          }
          if (v_lab > best2) {
            best2 = v_lab;
            bb2 = b_lab;
          }
          v_lab = best + r_lab;
          b_lab = v_lab == -INFINITY ? -1 : bb;
          v_blk = tail ? -INFINITY : best2 + r_blk;
          b_blk = v_blk == -INFINITY ? -1 : bb2;
          if (owner) {
            if (c_e >= 0 && ta - c_e >= hold) emit();
            if (v_lab >= thr && v_lab > -INFINITY) {
              if (c_e < 0 || v_lab > c_s || (v_lab == c_s && b_lab == c_b)) {
                c_s = v_lab;
                c_b = b_lab;
                c_e = ta;
              }
            }
            if (v_lab > m_s) {
              m_s = v_lab;
              m_b = b_lab;
              m_e = ta;
            }
          }
        }
      }
#pragma unroll
      for (int k = 0; k < KW_AHEAD; ++k) {
        pe[k] = ne[k];
        pb[k] = nb[k];
        pm[k] = nm[k];
      }
    }
    ls[0] = v_lab;
    ls[64] = v_blk;
    ls[128] = __int_as_float(b_lab);
    ls[192] = __int_as_float(b_blk);
    if (lane == 0) frm[(long)n * W + w] = t_base + size;
  }
  if (owner) {
    if (ending && c_e >= 0) emit();
    *reinterpret_cast<int4*>(ks) = make_int4(__float_as_int(c_s), c_b, c_e, __float_as_int(m_s));
    *reinterpret_cast<int4*>(ks + 4) = make_int4(m_b, m_e, 0, 0);
    hit_cnt[nk] = cnt;
  }
}

// out row of stream n: [hits, dropped, frames, 0] then the hits as (keyword, start, end, score bits), keyword-major, time order
// within a keyword; a keyword contributes its first min(count, max_hits) hits of this feed, the others are counted as dropped
__global__ void __launch_bounds__(256) k_kws_compact(const int* __restrict__ hit_cnt, const int* __restrict__ hits, int K, int max_hits,
                                                     const int* __restrict__ frm, int W, int* __restrict__ out, long out_stride) {
  __shared__ int wsum[4], wdrop[4];
  const int n = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  int* row = out + (long)n * out_stride;
  int base = 0, drop = 0;
  for (int k0 = 0; k0 < K; k0 += 256) {                    // uniform
    const int k = k0 + tid;
    int raw = k < K ? hit_cnt[(long)n * K + k] : 0;
    raw = raw < 0 ? 0 : raw;
    const int c = raw < max_hits ? raw : max_hits;
    int inc = c, d = raw - c;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int y = __shfl_up(inc, o, 64);
      if (lane >= o) inc += y;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) d += __shfl_xor(d, o, 64);
    if (lane == 63) {
      wsum[wv] = inc;
      wdrop[wv] = d;
    }
    __syncthreads();
    int off = base;
    for (int j = 0; j < wv; ++j) off += wsum[j];
    off += inc - c;
    const int* src = hits + ((long)n * K + k) * max_hits * 3;
    for (int j = 0; j < c; ++j)
      *reinterpret_cast<int4*>(row + KW_HDR + (long)(off + j) * KW_HIT_WORDS) = make_int4(k, src[j * 3], src[j * 3 + 1], src[j * 3 + 2]);
    base += wsum[0] + wsum[1] + wsum[2] + wsum[3];
    drop += wdrop[0] + wdrop[1] + wdrop[2] + wdrop[3];
    __syncthreads();
  }
  if (tid == 0) *reinterpret_cast<int4*>(row) = make_int4(base, drop, frm[(long)n * W], 0);
}

__global__ void __launch_bounds__(256) k_kws_reset(float* __restrict__ lat, int* __restrict__ key, int* __restrict__ frm, int W, int K,
                                                   const int* __restrict__ mask) {
  const int n = blockIdx.x;
  if (mask && mask[n] == 0) return;
  const int ninf = __float_as_int(-INFINITY);
  int* l = reinterpret_cast<int*>(lat) + (long)n * W * (KW_LAT_WORDS * 64);
  for (int i = threadIdx.x; i < W * KW_LAT_WORDS * 64; i += 256) l[i] = ((i >> 6) & 3) < 2 ? ninf : -1;
  int4* kk = reinterpret_cast<int4*>(key + (long)n * K * KW_KEY_WORDS);
  for (int i = threadIdx.x; i < 2 * K; i += 256) kk[i] = (i & 1) ? make_int4(-1, -1, 0, 0) : make_int4(ninf, -1, -1, ninf);
  for (int i = threadIdx.x; i < W; i += 256) frm[(long)n * W + i] = 0;
}

}  // namespace

extern "C" {

long ds2_kws_state_bytes(int N, int waves, int K) {
  if (N < 1 || waves < 1 || K < 1) return -1;
  return ((kw_lat_words(N, waves) + kw_key_words(N, K) + (long)N * waves) * 4 + 15) & ~15l;
}

long ds2_kws_ws_bytes(int N, int Tc, int K, int max_hits) {
  if (N < 1 || Tc < 0 || K < 1 || max_hits < 1 || max_hits > KW_MAX_HITS) return -1;
  return (kw_ws_fmax_words(N, Tc) + (long)N * K + (long)N * K * max_hits * 3) * 4;
}

long ds2_kws_out_stride(int K, int max_hits) {
  if (K < 1 || max_hits < 1 || max_hits > KW_MAX_HITS) return -1;
  return KW_HDR + (long)K * max_hits * KW_HIT_WORDS;
}

int ds2_kws_reset(void* state, int N, int waves, int K, const int* mask, ds2_stream_t st_) {
  DS2_REQUIRE(state && N > 0 && waves > 0 && K > 0, DS2_ERR_ARG);
  DS2_REQUIRE(((uintptr_t)state & 15) == 0, DS2_ERR_ALIGN);
  const KwState s = kw_state(state, N, waves, K);
  hipLaunchKernelGGL(k_kws_reset, dim3(N), dim3(256), 0, (hipStream_t)st_, s.lat, s.key, s.frm, waves, K, mask);
  DS2_CHECK_LAUNCH();
  return 0;
}

int ds2_kws_feed(const float* x, long stride_n, long stride_t, int N, int Tc, int C, int mode, const int* sizes, int blank,
                 const int* lanes, int waves, int K, int hold, int max_hits, const int* end_mask, int end_all, void* state, int* out,
                 void* ws, ds2_stream_t st_) {
  hipStream_t st = (hipStream_t)st_;
  DS2_REQUIRE(N > 0 && N <= KW_MAX_STREAMS && Tc >= 0 && C > 0 && blank >= 0 && blank < C && mode >= 0 && mode <= 2, DS2_ERR_ARG);
  DS2_REQUIRE(waves > 0 && K > 0 && hold >= 1 && max_hits >= 1 && max_hits <= KW_MAX_HITS, DS2_ERR_ARG);
  DS2_REQUIRE((x || Tc == 0) && lanes && state && out && ws, DS2_ERR_ARG);
  DS2_REQUIRE(((uintptr_t)state & 15) == 0 && ((uintptr_t)out & 15) == 0 && ((uintptr_t)lanes & 15) == 0 && ((uintptr_t)ws & 15) == 0,
              DS2_ERR_ALIGN);
  const KwState s = kw_state(state, N, waves, K);
  float* fmax = static_cast<float*>(ws);
  int* hit_cnt = reinterpret_cast<int*>(fmax + kw_ws_fmax_words(N, Tc));
  int* hits = hit_cnt + (long)N * K;
  if (Tc > 0) {
    if (C <= 256)
      hipLaunchKernelGGL(k_kws_framemax, dim3(ds2_cdiv((long)N * Tc, 256)), dim3(256), 0, st, x, stride_n, stride_t, sizes, Tc, N, C, mode,
                         fmax);
    else
      hipLaunchKernelGGL(k_kws_framemax_big, dim3(ds2_cdiv((long)N * Tc, 4)), dim3(256), 0, st, x, stride_n, stride_t, sizes, Tc, N, C,
                         mode, fmax);
    DS2_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(k_kws_lattice, dim3(ds2_cdiv(waves, KW_WPB), N), dim3(KW_WPB * 64), 0, st, x, stride_n, stride_t, Tc, C, mode, sizes,
                     blank, reinterpret_cast<const int4*>(lanes), waves, K, hold, max_hits, end_mask, end_all, s.lat, s.key, s.frm, fmax,
                     hit_cnt, hits);
  DS2_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_kws_compact, dim3(N), dim3(256), 0, st, hit_cnt, hits, K, max_hits, s.frm, waves, out,
                     KW_HDR + (long)K * max_hits * KW_HIT_WORDS);
  DS2_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
