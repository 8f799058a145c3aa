// CTC prefix beam search on the device, without a language model: the beam counterpart of ds2_decode.hip, behind
// decoder.BeamCTCDecoder (the interface of the reference's BeamCTCDecoder, decoder.py:56-117, which wraps the ctcdecode C++
// library and runs it in CPU threads on a host copy of the whole (N, T', C) probability tensor).  The rules are those of
// ctcdecode's ctc_beam_search_decoder without a scorer, as restated in DESIGN.md ("ds2_beam") and in tests/beam_reference.py.
//
// Two launches on the caller's stream:
//  k_beam_prune   one wave per (sample, frame): the classes kept in that frame, sorted by probability (descending, lower class
//                 first on ties), cut at cutoff_top_n and, with cutoff_prob < 1, at the first class where the cumulative
//                 probability (summed in fp64, in that order) reaches cutoff_prob; each with lp = log(p + FLT_MIN) (fp64, rounded to
//                 fp32).  K rounds of a wave arg-max over "the classes after the previous pick"; every frame in parallel, off the serial path.
//  k_beam_search  one workgroup (256 threads) per sample, one step per frame; the beam state lives in LDS, double-buffered.
//                 Per step:
//                   P1  kept list of frame t into LDS (prefetched into registers during step t-1), class -> slot map, every
//                       beam into an open-addressing table keyed by (hash of its label string, length)
//                   P2  one thread per (beam i, kept non-blank class c): the extension i+c; if the table holds a beam j with
//                       hash(j) == hash(i)*P + c + 1 and len(j) == len(i)+1, the mass goes to j (merge by string equality, so a
//                       prefix that was pruned and re-created merges with children that still hang off its old node) and j's
//                       last label may move to frame t (the log_prob_c rule); otherwise it is a new candidate
//                   P3  one thread per beam: the beam itself as a candidate (blank, repeated last label, merged extension)
//                   P4  top-B of all finite candidates: radix select, 8 bits a pass, on the 64-bit key
//                       (order-preserving score bits, ~(source rank << 14 | class + 1)); keys are unique, so the selected set
//                       and the tie rule (lower source rank, then lower class, the beam itself before its extensions) are exact
//                   P5  compaction of the selected candidates; P6 rank = number of larger keys, new state at that rank; a new
//                       string appends the node (parent, label, frame) at slot t*B + rank of the sample's node pool
//                 At the end one thread per beam walks the parent links and writes labels and frames.
// Workspace (torch-owned, ds2_beam_ws_bytes): the kept lists [N][T][64] and the node pool [N][T+1][B] x (parent, label, frame).
// A candidate's score is formed in one place per kind (the extension in P2, the beam itself in P3): a language-model bonus and
// a word-boundary hook at the space label would enter there, with pb / pnb kept as the acoustic part.
#include <float.h>

#include "ds2_common.h"

#define BEAM_MAXB 256
#define BEAM_MAXK 64
#define BEAM_MAXC 8192
#define BEAM_THREADS 256
#define BEAM_TABLE 512   // >= 2 * BEAM_MAXB: load factor <= 1/2
#define BEAM_TIE_CLASS_BITS 14

namespace {

constexpr uint64_t kM61 = (1ull << 61) - 1;          // prime modulus of the string hash
constexpr uint64_t kHashBase = 0x0b7e151628aed2a7ull;  // fixed base < kM61
constexpr uint64_t kHashEmpty = 0x1f3d5b79a2c4e6f8ull % kM61;

// hash(s + c) = (hash(s) * base + c + 1) mod (2^61 - 1)
__device__ __forceinline__ uint64_t hash_ext(uint64_t h, int c) {
  const uint64_t lo = h * kHashBase, hi = __umul64hi(h, kHashBase);
  uint64_t r = (lo & kM61) + ((lo >> 61) | (hi << 3));
  r = (r & kM61) + (r >> 61);
  r += (uint64_t)(c + 1);
  r = (r & kM61) + (r >> 61);
  return r >= kM61 ? r - kM61 : r;
}

__device__ __forceinline__ int hash_slot(uint64_t h, int len) {
  return (int)(((uint32_t)h ^ (uint32_t)(h >> 29) ^ ((uint32_t)len * 0x9e3779b9u)) & (BEAM_TABLE - 1));
}

// log(exp(x) + exp(y)) of two fp32 values, evaluated in fp64 and rounded once: the result is the correctly rounded fp32 value
// except in the rare double-rounding case, so a host restatement (numpy fp64, then fp32) reproduces it bit for bit.
__device__ __forceinline__ float lse(float x, float y) {
  if (x == -INFINITY) return y;
  if (y == -INFINITY) return x;
  const double m = (double)fmaxf(x, y);
  return (float)(m + log(exp((double)x - m) + exp((double)y - m)));
}

// order-preserving bits of a finite float: larger float -> larger unsigned
__device__ __forceinline__ uint32_t ord_bits(float f) {
  const uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// ---- per-frame pruning --------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_beam_prune(const float* __restrict__ x, long stride_n, long stride_t, int N, int T, int C,
                                                    const int* __restrict__ sizes, int K, int use_cut, double cutoff_prob,
                                                    int* __restrict__ pcnt, int* __restrict__ pcls, float* __restrict__ plp) {
  const int lane = threadIdx.x & 63;
  const long f = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (f >= (long)N * T) return;
  const int n = (int)(f / T), t = (int)(f - (long)n * T);
  int size = sizes ? sizes[n] : T;
  size = size < 0 ? 0 : (size > T ? T : size);
  if (t >= size) return;
  const float* row = x + (long)n * stride_n + (long)t * stride_t;
  int* cls = pcls + f * BEAM_MAXK;
  float* lps = plp + f * BEAM_MAXK;
  float pv = INFINITY;   // previous pick: value, class (the next pick comes after it in (value desc, class asc) order)
  int pi = -1;
  double cum = 0.0;
  int kept = 0;
  for (int r = 0; r < K; ++r) {
    float bv = -INFINITY;
    int bi = C;            // "none" (sorts after every class)
    for (int c = lane; c < C; c += 64) {
      const float v = row[c];
      const bool after = v < pv || (v == pv && c > pi);
      if (after && (v > bv || bi == C)) {   // ascending c within a lane: the first maximum wins
        bv = v;
        bi = c;
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(bv, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      if (oi != C && (bi == C || ov > bv || (ov == bv && oi < bi))) {
        bv = ov;
        bi = oi;
      }
    }
    if (bi == C) break;    // fewer orderable values than K (NaN rows): keep what was found
    if (lane == 0) {
      cls[r] = bi;
      lps[r] = (float)log((double)bv + (double)FLT_MIN);   // ctcdecode: log(prob + FLT_MIN) in fp64, kept as fp32
    }
    kept = r + 1;
    pv = bv;
    pi = bi;
    cum += (double)bv;
    if (use_cut && cum >= cutoff_prob) break;
  }
  if (lane == 0) pcnt[f] = kept;
}

// ---- the search ---------------------------------------------------------------------------------------------------------
struct BeamState {
  float pb[BEAM_MAXB], pnb[BEAM_MAXB], lpc[BEAM_MAXB];   // log P(ending in blank / non-blank); lp that set the last label's frame
  uint64_t hash[BEAM_MAXB];
  int len[BEAM_MAXB], last[BEAM_MAXB], node[BEAM_MAXB];  // last = -1 and node = -1 for the empty string
};

__device__ __forceinline__ int table_find(const int* table, const BeamState& S, uint64_t h, int len) {
  int slot = hash_slot(h, len);
  for (int probe = 0; probe < BEAM_TABLE; ++probe) {
    const int j = table[slot];
    if (j < 0) return -1;
    if (S.hash[j] == h && S.len[j] == len) return j;
    slot = (slot + 1) & (BEAM_TABLE - 1);
  }
  return -1;
}

__device__ __forceinline__ uint64_t cand_key(float s, int i, int cls1) {
  return ((uint64_t)ord_bits(s) << 32) | (uint32_t)~(((uint32_t)i << BEAM_TIE_CLASS_BITS) | (uint32_t)cls1);
}

__global__ void __launch_bounds__(BEAM_THREADS) k_beam_search(int T, int C, const int* __restrict__ sizes, int blank, int B, int K,
                                                              const int* __restrict__ pcnt, const int* __restrict__ pcls,
                                                              const float* __restrict__ plp, int* __restrict__ parent_,
                                                              int* __restrict__ label_, int* __restrict__ frame_,
                                                              int* __restrict__ tokens, int* __restrict__ offsets,
                                                              int* __restrict__ lens, float* __restrict__ scores) {
  __shared__ BeamState st[2];
  __shared__ int table[2][BEAM_TABLE];
  __shared__ float score[BEAM_MAXB], stay_pb[BEAM_MAXB], stay_pnb[BEAM_MAXB], ext_mass[BEAM_MAXB], new_lpc[BEAM_MAXB];
  __shared__ float cs[BEAM_MAXB * (BEAM_MAXK + 1)];    // candidate scores: beam i itself at i*W, extension (i, k) at i*W + 1 + k
  __shared__ short kidx[BEAM_MAXC];                    // class -> slot in this frame's kept list, -1 when not kept
  __shared__ int kc[BEAM_MAXK];
  __shared__ float klp[BEAM_MAXK];
  __shared__ unsigned hist[256];
  __shared__ uint64_t sel_key[BEAM_MAXB];
  __shared__ int sel_q[BEAM_MAXB];
  __shared__ int s_nsel, s_done;
  __shared__ uint64_t s_prefix, s_mask;
  __shared__ unsigned s_need;

  const int n = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  int size = sizes ? sizes[n] : T;
  size = size < 0 ? 0 : (size > T ? T : size);
  const long fbase = (long)n * T;
  const long pool = (long)n * (T + 1) * B;
  int* parent = parent_ + pool;
  int* label = label_ + pool;
  int* frame = frame_ + pool;

  for (int c = tid; c < C; c += BEAM_THREADS) kidx[c] = -1;
  for (int s = tid; s < 2 * BEAM_TABLE; s += BEAM_THREADS) (&table[0][0])[s] = -1;
  if (tid == 0) {
    st[0].pb[0] = 0.f;
    st[0].pnb[0] = -INFINITY;
    st[0].lpc[0] = -INFINITY;
    st[0].hash[0] = kHashEmpty;
    st[0].len[0] = 0;
    st[0].last[0] = -1;
    st[0].node[0] = -1;
  }
  int nb = 1, cur = 0;
  // kept list of the next frame, in registers of wave 0 (lane k holds slot k)
  int pf_cnt = 0, pf_c = 0;
  float pf_lp = 0.f;
  if (size > 0) {
    pf_cnt = pcnt[fbase];
    if (tid < K) {
      pf_c = pcls[fbase * BEAM_MAXK + tid];
      pf_lp = plp[fbase * BEAM_MAXK + tid];
    }
  }
  __syncthreads();

  for (int t = 0; t < size; ++t) {
    const BeamState& S = st[cur];
    BeamState& D = st[cur ^ 1];
    // ---- P1
    const int nk = pf_cnt < 1 ? 1 : (pf_cnt > K ? K : pf_cnt);   // >= 1 for every pruned frame; clamped against a bad count
    const int W = nk + 1;
    if (tid < nk) {
      const int c = pf_c < 0 ? 0 : (pf_c >= C ? C - 1 : pf_c);
      kc[tid] = c;
      klp[tid] = pf_lp;
      kidx[c] = (short)tid;
    }
    if (tid < nb) {
      int slot = hash_slot(S.hash[tid], S.len[tid]);
      for (int probe = 0; probe < BEAM_TABLE; ++probe) {
        if (atomicCAS(&table[cur][slot], -1, tid) == -1) break;
        slot = (slot + 1) & (BEAM_TABLE - 1);
      }
      score[tid] = lse(S.pb[tid], S.pnb[tid]);
      ext_mass[tid] = -INFINITY;
      new_lpc[tid] = S.lpc[tid];
    }
    for (int s = tid; s < BEAM_TABLE; s += BEAM_THREADS) table[cur ^ 1][s] = -1;
    if (tid == 0) s_nsel = 0;
    __syncthreads();
    // prefetch the next frame's kept list (hidden behind this step)
    if (t + 1 < size) {
      pf_cnt = pcnt[fbase + t + 1];
      if (tid < K) {
        pf_c = pcls[(fbase + t + 1) * BEAM_MAXK + tid];
        pf_lp = plp[(fbase + t + 1) * BEAM_MAXK + tid];
      }
    }
    // ---- P2: extensions
    for (int q = tid; q < nb * nk; q += BEAM_THREADS) {
      const int i = q / nk, k = q - i * nk;
      const int c = kc[k];
      const float lp = klp[k];
      float s = -INFINITY;
      if (c != blank) {
        const float mass = (c == S.last[i] ? S.pb[i] : score[i]) + lp;
        const int j = table_find(table[cur], S, hash_ext(S.hash[i], c), S.len[i] + 1);
        if (j >= 0) {          // i+c is beam j: the only source of an extension into j
          ext_mass[j] = mass;
          if (lp > S.lpc[j]) {
            new_lpc[j] = lp;
            frame[S.node[j]] = t;
          }
        } else {
          s = mass;
        }
      }
      cs[i * W + 1 + k] = s;
    }
    __syncthreads();
    // ---- P3: every beam itself
    if (tid < nb) {
      const int i = tid;
      const float pnb = S.pnb[i];
      const int kb = kidx[blank];
      const float npb = kb >= 0 ? score[i] + klp[kb] : -INFINITY;
      const int kl = S.last[i] >= 0 ? kidx[S.last[i]] : -1;
      float npnb = kl >= 0 ? pnb + klp[kl] : -INFINITY;
      npnb = lse(npnb, ext_mass[i]);
      stay_pb[i] = npb;
      stay_pnb[i] = npnb;
      cs[i * W] = lse(npb, npnb);
    }
    __syncthreads();
    // ---- P4: radix select of the B largest keys among the finite candidates
    const int Q = nb * W;
    uint64_t prefix = 0, mask = 0;
    unsigned need = (unsigned)B;
    for (int pass = 0; pass < 8; ++pass) {
      const int shift = 56 - 8 * pass;
      hist[tid] = 0;   // BEAM_THREADS == 256 bins
      __syncthreads();
      for (int q = tid; q < Q; q += BEAM_THREADS) {
        const float s = cs[q];
        if (s == -INFINITY) continue;
        const int i = q / W, m = q - i * W;
        const uint64_t key = cand_key(s, i, m == 0 ? 0 : kc[m - 1] + 1);
        if ((key & mask) == prefix) atomicAdd(&hist[(key >> shift) & 255], 1u);
      }
      __syncthreads();
      if (tid < 64) {
        // lane l: bins 255-4l .. 252-4l (largest digits first)
        unsigned h4[4], sum = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          h4[j] = hist[255 - 4 * lane - j];
          sum += h4[j];
        }
        unsigned cum = sum;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
          const unsigned v = __shfl_up(cum, o, 64);
          if (lane >= o) cum += v;
        }
        const unsigned total = __shfl(cum, 63, 64);
        if (pass == 0 && total <= need) {
          if (lane == 0) {
            s_prefix = 0;
            s_mask = 0;
            s_done = 1;
          }
        } else {
          const unsigned long long hit = __ballot(cum >= need);
          const int L = __ffsll((long long)hit) - 1;   // total > need (pass 0) or >= need (later passes): hit != 0
          if (lane == L) {
            unsigned before = cum - sum;
            int d = 255 - 4 * lane - 3;
            unsigned take = need - before;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              if (before + h4[j] >= need) {
                d = 255 - 4 * lane - j;
                take = need - before;
                break;
              }
              before += h4[j];
            }
            s_prefix = prefix | ((uint64_t)d << shift);
            s_mask = mask | (255ull << shift);
            s_need = take;
            s_done = hist[d] == take;
          }
        }
      }
      __syncthreads();
      prefix = s_prefix;
      mask = s_mask;
      need = s_need;
      if (s_done) break;
    }
    // ---- P5: compaction of the selected candidates (key & mask >= prefix)
    for (int q = tid; q < Q; q += BEAM_THREADS) {
      const float s = cs[q];
      if (s == -INFINITY) continue;
      const int i = q / W, m = q - i * W;
      const uint64_t key = cand_key(s, i, m == 0 ? 0 : kc[m - 1] + 1);
      if ((key & mask) >= prefix) {
        const int slot = atomicAdd(&s_nsel, 1);
        if (slot < B) {
          sel_key[slot] = key;
          sel_q[slot] = q;
        }
      }
    }
    __syncthreads();
    // ---- P6: ranks and the next state
    const int ns = s_nsel < B ? s_nsel : B;
    if (tid < ns) {
      const uint64_t key = sel_key[tid];
      int r = 0;
      for (int s = 0; s < ns; ++s) r += sel_key[s] > key;
      const int q = sel_q[tid];
      const int i = q / W, m = q - i * W;
      if (m == 0) {
        D.pb[r] = stay_pb[i];
        D.pnb[r] = stay_pnb[i];
        D.lpc[r] = new_lpc[i];
        D.hash[r] = S.hash[i];
        D.len[r] = S.len[i];
        D.last[r] = S.last[i];
        D.node[r] = S.node[i];
      } else {
        const int c = kc[m - 1];
        const int id = t * B + r;
        D.pb[r] = -INFINITY;
        D.pnb[r] = cs[q];
        D.lpc[r] = klp[m - 1];
        D.hash[r] = hash_ext(S.hash[i], c);
        D.len[r] = S.len[i] + 1;
        D.last[r] = c;
        D.node[r] = id;
        parent[id] = S.node[i];
        label[id] = c;
        frame[id] = t;
      }
    }
    if (tid < nk) kidx[kc[tid]] = -1;
    nb = ns;
    cur ^= 1;
    __syncthreads();
  }

  // ---- output: one thread per rank walks the parent links
  __threadfence();
  __syncthreads();
  __threadfence();
  const BeamState& S = st[cur];
  if (tid < B) {
    const long o = (long)n * B + tid;
    if (tid < nb) {
      const int len = S.len[tid];
      int node = S.node[tid];
      int* tok = tokens + o * T;
      int* off = offsets + o * T;
      for (int pos = len - 1; pos >= 0 && node >= 0; --pos) {
        tok[pos] = label[node];
        off[pos] = frame[node];
        node = parent[node];
      }
      lens[o] = len;
      scores[o] = -lse(S.pb[tid], S.pnb[tid]) + 0.f;
    } else {
      lens[o] = 0;
      scores[o] = INFINITY;
    }
  }
}

long align256(long b) { return (b + 255) / 256 * 256; }

struct WsLayout {
  long cnt, cls, lp, parent, label, frame, total;
};

WsLayout ws_layout(int N, int T, int B) {
  WsLayout L;
  const long frames = (long)N * T, nodes = (long)N * (T + 1) * B;
  L.cnt = 0;
  L.cls = L.cnt + align256(frames * 4);
  L.lp = L.cls + align256(frames * BEAM_MAXK * 4);
  L.parent = L.lp + align256(frames * BEAM_MAXK * 4);
  L.label = L.parent + align256(nodes * 4);
  L.frame = L.label + align256(nodes * 4);
  L.total = L.frame + align256(nodes * 4);
  return L;
}

}  // namespace

extern "C" {

long ds2_beam_ws_bytes(int N, int T, int B) {
  if (N <= 0 || T <= 0 || B <= 0) return 0;
  return ws_layout(N, T, B).total;
}

// x: probabilities of sample n, frame t, class c at x[n*stride_n + t*stride_t + c] (f32, class dimension contiguous).
// sizes: [N] valid frames (device int32, null = T).  Outputs (device): tokens / offsets [N][B][T] int32 (the first lens[n][b]
// entries of row (n, b) are valid), lens [N][B] int32, scores [N][B] f32 (-log p, +inf for a rank with no beam).
// ws: ds2_beam_ws_bytes(N, T, B) bytes, 256-byte aligned.
int ds2_beam_decode(const float* x, long stride_n, long stride_t, int N, int T, int C, const int* sizes, int blank, int B,
                    int cutoff_top_n, float cutoff_prob, int* tokens, int* offsets, int* lens, float* scores, void* ws,
                    ds2_stream_t st_) {
  hipStream_t st = (hipStream_t)st_;
  DS2_REQUIRE(N > 0 && T > 0 && C > 0 && C <= BEAM_MAXC && blank >= 0 && blank < C, DS2_ERR_ARG);
  DS2_REQUIRE(B >= 1 && B <= BEAM_MAXB && cutoff_top_n >= 1, DS2_ERR_ARG);
  const int K = cutoff_top_n < C ? cutoff_top_n : C;
  DS2_REQUIRE(K <= BEAM_MAXK, DS2_ERR_ARG);
  DS2_REQUIRE(x && tokens && offsets && lens && scores && ws, DS2_ERR_ARG);
  DS2_REQUIRE(((uintptr_t)ws & 255) == 0, DS2_ERR_ALIGN);
  const WsLayout L = ws_layout(N, T, B);
  char* w = (char*)ws;
  int* pcnt = (int*)(w + L.cnt);
  int* pcls = (int*)(w + L.cls);
  float* plp = (float*)(w + L.lp);
  const int use_cut = cutoff_prob < 1.0f;
  const long frames = (long)N * T;
  hipLaunchKernelGGL(k_beam_prune, dim3((unsigned)((frames + 3) / 4)), dim3(256), 0, st, x, stride_n, stride_t, N, T, C, sizes, K,
                     use_cut, (double)cutoff_prob, pcnt, pcls, plp);
  DS2_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_beam_search, dim3(N), dim3(BEAM_THREADS), 0, st, T, C, sizes, blank, B, K, pcnt, pcls, plp,
                     (int*)(w + L.parent), (int*)(w + L.label), (int*)(w + L.frame), tokens, offsets, lens, scores);
  DS2_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
