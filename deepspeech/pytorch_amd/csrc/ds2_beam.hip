// CTC prefix beam search on the device, with or without a word n-gram language model: the beam counterpart of ds2_decode.hip, behind
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
// A candidate's score is formed in one place per kind (the extension in P2, the beam itself in P3).
//
// k_beam_search<true> (ds2_beam_decode_lm) adds the language model of DESIGN.md "ds2_beam": what the selection compares is
// lse(pb, pnb) + lm, with pb / pnb kept as the acoustic part.  A beam carries lm (the fp32 sum of its word bonuses), the hash of its
// partial word (the labels after its last space), the id of that word, the ids of its last order - 1 completed words, and its
// space bonus: what an extension by the space label adds to lm.  The space bonus depends on the string alone, so it is
// computed once, in P6, when the string is created: one probe of the word table for the id, then the n-gram probes of all suffix
// orders and their contexts together.  P2 only adds lm (plus the space bonus at the space label); in lexicon mode it probes the
// word table once per new candidate and drops the ones that spell no word prefix.  The tables are built on the host (lm.py).
// k_beam_search<false> is the code without any of it: every addition sits under `if constexpr (LM)`, and the LM state and
// arguments exist only in the LM instantiation.
// k_beam_search<true, LmArgs, GridArgs> (ds2_beam_decode_lm_grid) is the LM search on (N, G) workgroups for G weight points: one
// prune launch, workgroup (n, g) takes alphas[g] / betas[g] and node pool g, and writes its top beam only.
// k_beam_search<false, StreamArgs> / <true, LmArgs, StreamArgs> (ds2_beam_stream_feed / _feed_lm) is the resumable search: workgroup
// n loads the state of stream n (nb, BeamState, LmState) from a device buffer, runs this chunk's frames numbered from the start of
// the stream in a node pool that outlives the launch, and stores the state back; the output stage is optional and changes nothing.
// k_beam_search<false, HotArgs> / <true, LmArgs, HotArgs>, and both with StreamArgs last (ds2_beam_decode_hot, _lm_hot,
// ds2_beam_stream_feed_hot, _feed_lm_hot) add the hot words of DESIGN.md "ds2_beam": what the selection compares gains hot = done
// + v(match), from a second per-beam state (HotState) that is a function of the string alone.  P2 probes the phrase table with
// two keys at once per new candidate, P6 repeats that for a new string and probes once more for its space extension.  Every
// addition sits under `if constexpr (HOT)`; the six instantiations above compile to the instructions they had without it.
// k_beam_search<false, ClmArgs>, <false, ClmArgs, StreamArgs>, <false, ClmArgs, GridArgs> (ds2_beam_decode_clm,
// ds2_beam_stream_feed_clm, ds2_beam_decode_clm_grid) score with a character n-gram model (DESIGN.md "ds2_beam", character language
// model): every new candidate of P2 is an event of the model, probed there; a beam carries lm, its last order - 1 label ids and the
// backoffs of its context suffixes (ClmState, probed once in P6), and there is no end-of-utterance term.  Every addition sits under
// `if constexpr (CLM)`; the ten instantiations above compile to the instructions they had without it.
#include <float.h>

#include "ds2_common.h"
#include "ds2_strhash.h"

#define BEAM_MAXB 256
#define BEAM_MAXK 64
#define BEAM_MAXC 8192
#define BEAM_THREADS 256
#define BEAM_TABLE 512   // >= 2 * BEAM_MAXB: load factor <= 1/2
#define BEAM_TIE_CLASS_BITS 14
#define BEAM_LM_MAX_ORDER 5
#define BEAM_MAX_POINTS 65535   // grid dimension y

namespace {

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

// ---- language model ------------------------------------------------------------------------------------------------------
constexpr uint64_t kTabEmpty = ~0ull;                  // free slot of both tables
constexpr uint64_t kNgramSeed = 0x243f6a8885a308d3ull;
constexpr uint64_t kNgramMul = 0x9e3779b97f4a7c15ull;
constexpr double kLog10e = 0.4342944819032518;
constexpr double kOovScore = -1000.0;                  // ln P of a word event with an unknown word or context
constexpr int kWordAbsent = -2;                        // word-table answers besides a word id; -1 = a proper prefix
constexpr int kHotWord = -2;                           // in a context (hot-word instantiations): a covered out-of-vocabulary hot word

struct LmArgs {
  const ulonglong2* wtab;   // word table [wmask + 1] x (key, value)
  const ulonglong2* gtab;   // n-gram table [gmask + 1] x (key, log10 p bits | log10 backoff bits << 32)
  unsigned wmask, gmask;
  int space, order, bos, lexicon;
  float alpha, beta;
  float* acoustic;          // [N][B] -lse(pb, pnb), or null
};

struct LmState {
  float lm[BEAM_MAXB], spb[BEAM_MAXB];                 // sum of the word bonuses; space bonus (-inf: no space extension)
  uint64_t whash[BEAM_MAXB];                           // partial word, kHashEmpty when there is none
  int wid[BEAM_MAXB];                                  // its word id, -1 when it is no vocabulary word
  int ctx[BEAM_LM_MAX_ORDER - 1][BEAM_MAXB];           // ctx[0] = the last completed word; -1 = out of vocabulary
};

__device__ __forceinline__ uint64_t ngram_mix(uint64_t h, int id) {
  const uint64_t t = (h ^ (uint64_t)(int64_t)(id + 1)) * kNgramMul;
  return t ^ (t >> 29);
}

__device__ __forceinline__ unsigned tab_slot(uint64_t key, unsigned mask) { return ((unsigned)key ^ (unsigned)(key >> 32)) & mask; }

// word id (>= 0), -1 for a proper prefix of a word, kWordAbsent
__device__ __forceinline__ int word_lookup(const LmArgs& A, uint64_t h) {
  unsigned slot = tab_slot(h, A.wmask);
  for (unsigned probe = 0; probe <= A.wmask; ++probe) {
    const ulonglong2 e = A.wtab[slot];
    if (e.x == h) return (int)(long long)e.y;
    if (e.x == kTabEmpty) return kWordAbsent;
    slot = (slot + 1) & A.wmask;
  }
  return kWordAbsent;
}

// alpha * ln P + beta, formed in fp64 without contraction and rounded once
__device__ __forceinline__ float lm_bonus(const LmArgs& A, double lnp) {
  return (float)__dadd_rn(__dmul_rn((double)A.alpha, lnp), (double)A.beta);
}

// The bonus of completing word w after the context c[0] (most recent), c[1], ...: backoff over the stored n-grams.  Keys of
// (c[m-1] .. c[0], w) for m = 0 .. order-1 and of the contexts (c[m] .. c[0]) for m = 0 .. order-2; all first probes are loaded
// before any is looked at, and a later probe round only serves the keys whose slot held another key.
// HOT (the hot-word instantiations): a context id may also be kHotWord, a covered out-of-vocabulary hot word.  It is not the
// out-of-vocabulary mark, and no key that would contain it is probed, so it matches no stored n-gram and its contexts add backoff 0.
template <bool HOT>
__device__ __forceinline__ float word_bonus(const LmArgs& A, int w, const int (&c)[BEAM_LM_MAX_ORDER - 1]) {
  constexpr int NP = 2 * BEAM_LM_MAX_ORDER - 1;   // 0 .. 4: n-grams ending in w; 5 .. 8: contexts
  bool oov = w < 0;
#pragma unroll
  for (int m = 0; m < BEAM_LM_MAX_ORDER - 1; ++m) oov |= m < A.order - 1 && (HOT ? c[m] == -1 : c[m] < 0);
  if (oov) return lm_bonus(A, kOovScore);
  uint64_t key[NP];
  unsigned slot[NP], pending = 0, found = 0;
  uint64_t val[NP];
  uint64_t h = ngram_mix(kNgramSeed, w), g = kNgramSeed;
  key[0] = h;
  pending = 1u;
  [[maybe_unused]] bool clean = true;             // no kHotWord among c[0 .. m]
#pragma unroll
  for (int m = 0; m < BEAM_LM_MAX_ORDER - 1; ++m) {
    h = ngram_mix(h, c[m]);
    g = ngram_mix(g, c[m]);
    key[m + 1] = h;
    key[BEAM_LM_MAX_ORDER + m] = g;
    if constexpr (HOT) {
      clean &= c[m] != kHotWord;
      if (m < A.order - 1 && clean) pending |= (1u << (m + 1)) | (1u << (BEAM_LM_MAX_ORDER + m));
    } else {
      if (m < A.order - 1) pending |= (1u << (m + 1)) | (1u << (BEAM_LM_MAX_ORDER + m));
    }
  }
#pragma unroll
  for (int j = 0; j < NP; ++j) {
    slot[j] = tab_slot(key[j], A.gmask);
    val[j] = 0;
  }
  for (unsigned probe = 0; probe <= A.gmask && pending; ++probe) {
    // every key loads, pending or not (a settled key reads its last slot again): no branch separates the loads, so they are in
    // flight together
    ulonglong2 e[NP];
#pragma unroll
    for (int j = 0; j < NP; ++j) e[j] = A.gtab[slot[j]];
#pragma unroll
    for (int j = 0; j < NP; ++j) {
      const bool open = pending >> j & 1, match = e[j].x == key[j], free_slot = e[j].x == kTabEmpty;
      val[j] = open && match ? e[j].y : val[j];
      found |= (unsigned)(open && match) << j;
      pending &= ~((unsigned)(open && (match || free_slot)) << j);
      slot[j] = open && !match && !free_slot ? (slot[j] + 1) & A.gmask : slot[j];
    }
  }
  // the longest stored n-gram ending in w; every shorter step adds the backoff of the context it drops (0 when not stored)
  double acc = 0.0;
  bool hit = false;
#pragma unroll
  for (int m = BEAM_LM_MAX_ORDER - 1; m >= 0; --m) {
    if (m < A.order && !hit) {
      if (found >> m & 1) {
        acc = __dadd_rn(acc, (double)__uint_as_float((unsigned)val[m]));
        hit = true;
      } else if (m > 0) {
        acc = __dadd_rn(acc, (double)__uint_as_float((unsigned)(val[BEAM_LM_MAX_ORDER + m - 1] >> 32)));
      }
    }
  }
  if (!hit) return lm_bonus(A, kOovScore);   // a word id without a unigram: not built by lm.py
  return lm_bonus(A, __ddiv_rn(acc, kLog10e));
}

// the LM instantiation's state lives in a function of its own, so that the plain instantiation never names it
__device__ __forceinline__ LmState* lm_state() {
  __shared__ LmState s[2];
  return s;
}

// ---- character language model --------------------------------------------------------------------------------------------
// DESIGN.md "ds2_beam", character language model: every label is an event of the n-gram model, so the model is charged for every
// new candidate in P2.  cid maps a class to its unigram id (-1: none).  A beam carries lm, the ids of its last order - 1 labels
// (ctx[0] the most recent, <s> in front of a short string, -1 the out-of-vocabulary mark) and the log10 backoffs of its context
// suffixes, bo[m] of (ctx[m] .. ctx[0]), 0 where that context is not stored: a function of the string alone, probed once in P6.
struct ClmArgs {
  const int* cid;           // [C] class -> unigram id, -1 when the file has none (the blank's entry is not read)
  const ulonglong2* gtab;   // n-gram table [gmask + 1] x (key, log10 p bits | log10 backoff bits << 32)
  unsigned gmask;
  int order, bos;
  float alpha, beta;
  float* acoustic;          // [N][B] -lse(pb, pnb), or null
};
struct NoClm {};

struct ClmState {
  float lm[BEAM_MAXB];                                 // sum of the label bonuses
  int ctx[BEAM_LM_MAX_ORDER - 1][BEAM_MAXB];
  float bo[BEAM_LM_MAX_ORDER - 1][BEAM_MAXB];
};
static_assert(sizeof(ClmState) == sizeof(LmState), "the character-LM state takes the room of the word-LM state");

// like lm_state(): only the character-LM instantiations name it
__device__ __forceinline__ ClmState* clm_state() {
  __shared__ ClmState s[2];
  return s;
}

__device__ __forceinline__ float clm_scale(const ClmArgs& A, double lnp) {
  return (float)__dadd_rn(__dmul_rn((double)A.alpha, lnp), (double)A.beta);
}

// NP keys of the n-gram table at once, as word_bonus probes: one unconditional round of loads, later rounds (bounded by the table
// size) only while a key is displaced.  Returns the mask of the keys found, their values in val.
template <int NP>
__device__ __forceinline__ unsigned clm_find(const ClmArgs& A, const uint64_t (&key)[NP], unsigned pending, uint64_t (&val)[NP]) {
  unsigned slot[NP], found = 0;
#pragma unroll
  for (int j = 0; j < NP; ++j) {
    slot[j] = tab_slot(key[j], A.gmask);
    val[j] = 0;
  }
  for (unsigned probe = 0; probe <= A.gmask && pending; ++probe) {
    ulonglong2 e[NP];
#pragma unroll
    for (int j = 0; j < NP; ++j) e[j] = A.gtab[slot[j]];
#pragma unroll
    for (int j = 0; j < NP; ++j) {
      const bool open = pending >> j & 1, match = e[j].x == key[j], free_slot = e[j].x == kTabEmpty;
      val[j] = open && match ? e[j].y : val[j];
      found |= (unsigned)(open && match) << j;
      pending &= ~((unsigned)(open && (match || free_slot)) << j);
      slot[j] = open && !match && !free_slot ? (slot[j] + 1) & A.gmask : slot[j];
    }
  }
  return found;
}

// The bonus of the label with unigram id w after the context c (c[0] the most recent) whose suffixes have the backoffs bo: the
// keys of (c[m-1] .. c[0], w), m = 0 .. order-1, are probed together; the longest stored one gives log10 p, and every shorter step
// above it first adds the backoff of the context it drops.
__device__ __forceinline__ float clm_bonus(const ClmArgs& A, int w, const int (&c)[BEAM_LM_MAX_ORDER - 1],
                                           const float (&bo)[BEAM_LM_MAX_ORDER - 1]) {
  bool oov = w < 0;
#pragma unroll
  for (int m = 0; m < BEAM_LM_MAX_ORDER - 1; ++m) oov |= m < A.order - 1 && c[m] < 0;
  if (oov) return clm_scale(A, kOovScore);
  uint64_t key[BEAM_LM_MAX_ORDER], val[BEAM_LM_MAX_ORDER];
  unsigned pending = 1u;
  uint64_t h = ngram_mix(kNgramSeed, w);
  key[0] = h;
#pragma unroll
  for (int m = 0; m < BEAM_LM_MAX_ORDER - 1; ++m) {
    h = ngram_mix(h, c[m]);
    key[m + 1] = h;
    if (m < A.order - 1) pending |= 1u << (m + 1);
  }
  const unsigned found = clm_find<BEAM_LM_MAX_ORDER>(A, key, pending, val);
  double acc = 0.0;
  bool hit = false;
#pragma unroll
  for (int m = BEAM_LM_MAX_ORDER - 1; m >= 0; --m) {
    if (m < A.order && !hit) {
      if (found >> m & 1) {
        acc = __dadd_rn(acc, (double)__uint_as_float((unsigned)val[m]));
        hit = true;
      } else if (m > 0) {
        acc = __dadd_rn(acc, (double)bo[m - 1]);
      }
    }
  }
  if (!hit) return clm_scale(A, kOovScore);   // an id without a unigram: not built by lm.py
  return clm_scale(A, __ddiv_rn(acc, kLog10e));
}

// the backoffs of the suffixes of the context c, for a new string: bo[m] of (c[m] .. c[0]), 0 when it is not stored or holds -1
__device__ __forceinline__ void clm_backoffs(const ClmArgs& A, const int (&c)[BEAM_LM_MAX_ORDER - 1],
                                             float (&bo)[BEAM_LM_MAX_ORDER - 1]) {
  uint64_t key[BEAM_LM_MAX_ORDER - 1], val[BEAM_LM_MAX_ORDER - 1];
  unsigned pending = 0;
  uint64_t g = kNgramSeed;
  bool known = true;
#pragma unroll
  for (int m = 0; m < BEAM_LM_MAX_ORDER - 1; ++m) {
    g = ngram_mix(g, c[m]);
    key[m] = g;
    known &= c[m] >= 0;
    if (m < A.order - 1 && known) pending |= 1u << m;
  }
  const unsigned found = clm_find<BEAM_LM_MAX_ORDER - 1>(A, key, pending, val);
#pragma unroll
  for (int m = 0; m < BEAM_LM_MAX_ORDER - 1; ++m) bo[m] = found >> m & 1 ? __uint_as_float((unsigned)(val[m] >> 32)) : 0.f;
}

// ---- hot words -----------------------------------------------------------------------------------------------------------
// DESIGN.md "ds2_beam", hot words.  The table (hotwords.py) has one entry for every non-empty prefix q of every phrase: key = the
// string hash of q (space label included), value = v(q) bits | c(q) bits << 32 | whole phrase << 63.  A beam carries the hash of its
// match mu (kHashEmpty: none), done, v(mu), what its space extension adds (hsv: c(mu) when mu is a whole phrase, else v(mu + space)
// when that is in the table, else 0) and two flags: bit 0 the space is covered, bit 1 mu is a whole phrase.  hot = done + v(mu);
// hot of the space extension = done + hsv; hot_end = done + hsv when mu is a whole phrase, else done.
struct HotArgs {
  const ulonglong2* htab;   // [hmask + 1] x (key, value)
  unsigned hmask;
  int space;
  float oov_logp;           // ln P charged to a covered out-of-vocabulary word event (LM instantiations)
  float* acoustic;          // [N][B] -lse(pb, pnb), or null (instantiations without an LM; with one LmArgs has it)
};
struct NoHot {};

struct HotState {
  uint64_t mh[BEAM_MAXB];
  float done[BEAM_MAXB], hv[BEAM_MAXB], hsv[BEAM_MAXB];
  int flags[BEAM_MAXB];
};
struct HotWord {
  uint64_t whash[BEAM_MAXB];                           // partial word (the LM instantiations have it in LmState)
};
constexpr int kHotCovered = 1, kHotComplete = 2;

// like lm_state(): only the hot-word instantiations name these
__device__ __forceinline__ HotState* hot_state() {
  __shared__ HotState s[2];
  return s;
}
__device__ __forceinline__ HotWord* hot_word() {
  __shared__ HotWord s[2];
  return s;
}

__device__ __forceinline__ float hot_v(uint64_t e) { return __uint_as_float((unsigned)e); }
__device__ __forceinline__ float hot_c(uint64_t e) { return __uint_as_float((unsigned)(e >> 32) & 0x7fffffffu); }

// NP keys at once, as word_bonus probes: every key loads in every round, open or not, so the loads are in flight together; the
// rounds are bounded by the table size.  Returns the mask of the keys found, their values in val.
template <int NP>
__device__ __forceinline__ unsigned hot_find(const HotArgs& H, const uint64_t (&key)[NP], unsigned pending, uint64_t (&val)[NP]) {
  unsigned slot[NP], found = 0;
#pragma unroll
  for (int j = 0; j < NP; ++j) {
    slot[j] = tab_slot(key[j], H.hmask);
    val[j] = 0;
  }
  for (unsigned probe = 0; probe <= H.hmask && pending; ++probe) {
    ulonglong2 e[NP];
#pragma unroll
    for (int j = 0; j < NP; ++j) e[j] = H.htab[slot[j]];
#pragma unroll
    for (int j = 0; j < NP; ++j) {
      const bool open = pending >> j & 1, match = e[j].x == key[j], free_slot = e[j].x == kTabEmpty;
      val[j] = open && match ? e[j].y : val[j];
      found |= (unsigned)(open && match) << j;
      pending &= ~((unsigned)(open && (match || free_slot)) << j);
      slot[j] = open && !match && !free_slot ? (slot[j] + 1) & H.hmask : slot[j];
    }
  }
  return found;
}

// the match of a string extended by the non-space label c: mu + c if the table has it (tried only when mu is not empty), else
// partial word + c (a match anchored at this word's start).  Both keys are probed together.  False: no match.
__device__ __forceinline__ bool hot_match(const HotArgs& H, uint64_t mh, uint64_t whash, int c, uint64_t& mh2, uint64_t& e) {
  const uint64_t key[2] = {hash_ext(mh, c), hash_ext(whash, c)};
  uint64_t val[2];
  const unsigned found = hot_find<2>(H, key, (mh != kHashEmpty ? 1u : 0u) | 2u, val);
  const bool first = found & 1u;
  mh2 = found ? (first ? key[0] : key[1]) : kHashEmpty;
  e = first ? val[0] : val[1];
  return found != 0;
}

// A grid of (alpha, beta) points (ds2_beam_decode_lm_grid): workgroup (n, g) searches sample n with the weights of point g in a
// node pool of its own, and only its top beam leaves the kernel.
struct GridArgs {
  const float* alphas;      // [G]
  const float* betas;       // [G]
  long pool_stride;         // nodes between the pools of two points
};

// what the kernel's trailing arguments say about the language model: nothing, the LmArgs, or the LmArgs with this point's weights
struct NoLm {};
__device__ __forceinline__ NoLm lm_args() { return {}; }
__device__ __forceinline__ LmArgs lm_args(const LmArgs& a) { return a; }
__device__ __forceinline__ LmArgs lm_args(const LmArgs& a, const GridArgs& g) {
  LmArgs r = a;
  r.alpha = g.alphas[blockIdx.y];
  r.beta = g.betas[blockIdx.y];
  return r;
}
__device__ __forceinline__ long grid_pool(const LmArgs&, const GridArgs& g) { return (long)blockIdx.y * g.pool_stride; }

// A resumable search (ds2_beam_stream_feed, ds2_beam_stream_feed_lm): workgroup n continues stream n from the state that the
// previous feed stored.  Per stream the state is a header of four ints (frames consumed, live beams nb, overflow flag, unused)
// followed by the beams' fields as arrays of B entries each: hash, pb, pnb, lpc, len, last, node, and with an LM whash, lm, spb, wid,
// ctx[0 .. 3].  The node pool [N][max_frames + 1][B] belongs to the session; frames, node slots and offsets count from the start of
// the stream.
struct StreamArgs {
  char* state;              // [N] x state_stride bytes
  long state_stride;
  int max_frames;
  long row_stride;          // ints between two rows of tokens / offsets (>= the largest consumed count)
  int out_ranks;            // the output stage writes the best out_ranks beams of every stream (1 .. B)
};
constexpr int kStreamHeader = 16;                      // bytes
constexpr int kStreamBeamBytes = 8 + 6 * 4;            // per beam: hash; pb, pnb, lpc, len, last, node
constexpr int kStreamLmBytes = 8 + (3 + BEAM_LM_MAX_ORDER - 1) * 4;   // whash; lm, spb, wid, ctx[]
constexpr int kStreamHotBytes = 8 + 4 * 4;             // mh; done, hv, hsv, flags -- and whash (8 more) where no LM stores it
// the hot-word fields follow the others at the next multiple of 8 bytes (the LM's fields are 36 bytes a beam)
__host__ __device__ constexpr long stream_hot_off(bool lm, long B) {
  return ((kStreamBeamBytes + (lm ? kStreamLmBytes : 0)) * B + 7) & ~7l;
}

__device__ __forceinline__ NoLm lm_args(const StreamArgs&) { return {}; }
__device__ __forceinline__ LmArgs lm_args(const LmArgs& a, const StreamArgs&) { return a; }
__device__ __forceinline__ const StreamArgs& stream_args(const StreamArgs& s) { return s; }
__device__ __forceinline__ const StreamArgs& stream_args(const LmArgs&, const StreamArgs& s) { return s; }

// the packs of the hot-word instantiations: [LmArgs,] HotArgs [, StreamArgs]
__device__ __forceinline__ NoLm lm_args(const HotArgs&) { return {}; }
__device__ __forceinline__ LmArgs lm_args(const LmArgs& a, const HotArgs&) { return a; }
__device__ __forceinline__ NoLm lm_args(const HotArgs&, const StreamArgs&) { return {}; }
__device__ __forceinline__ LmArgs lm_args(const LmArgs& a, const HotArgs&, const StreamArgs&) { return a; }
__device__ __forceinline__ const StreamArgs& stream_args(const HotArgs&, const StreamArgs& s) { return s; }
__device__ __forceinline__ const StreamArgs& stream_args(const LmArgs&, const HotArgs&, const StreamArgs& s) { return s; }
__device__ __forceinline__ NoHot hot_args() { return {}; }
template <class A, class... R>
__device__ __forceinline__ auto hot_args(const A& a, const R&... r) {
  if constexpr (__is_same(A, HotArgs)) return a;
  else return hot_args(r...);
}
template <class X, class... Extra> struct Has { static constexpr bool value = (__is_same(Extra, X) || ...); };

// the packs of the character-LM instantiations: ClmArgs [, GridArgs | StreamArgs], with LM = false
__device__ __forceinline__ NoLm lm_args(const ClmArgs&) { return {}; }
__device__ __forceinline__ NoLm lm_args(const ClmArgs&, const GridArgs&) { return {}; }
__device__ __forceinline__ NoLm lm_args(const ClmArgs&, const StreamArgs&) { return {}; }
__device__ __forceinline__ const StreamArgs& stream_args(const ClmArgs&, const StreamArgs& s) { return s; }
__device__ __forceinline__ long grid_pool(const ClmArgs&, const GridArgs& g) { return (long)blockIdx.y * g.pool_stride; }
template <class... R>
__device__ __forceinline__ NoClm clm_args(const R&...) { return {}; }
__device__ __forceinline__ ClmArgs clm_args(const ClmArgs& a) { return a; }
__device__ __forceinline__ ClmArgs clm_args(const ClmArgs& a, const StreamArgs&) { return a; }
__device__ __forceinline__ ClmArgs clm_args(const ClmArgs& a, const GridArgs& g) {
  ClmArgs r = a;
  r.alpha = g.alphas[blockIdx.y];
  r.beta = g.betas[blockIdx.y];
  return r;
}

// whether the last of the kernel's trailing argument types is X
template <class X, class... Extra> struct LastIs { static constexpr bool value = false; };
template <class X, class A> struct LastIs<X, A> { static constexpr bool value = __is_same(A, X); };
template <class X, class A, class B, class... Extra> struct LastIs<X, A, B, Extra...> : LastIs<X, B, Extra...> {};

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

// Extra is empty (LM = false), one LmArgs (LM = true), LmArgs, GridArgs (LM = true, launched as (N, G) workgroups), or either of
// the first two followed by StreamArgs (the resumable form)
template <bool LM, class... Extra>
__global__ void __launch_bounds__(BEAM_THREADS) k_beam_search(int T, int C, const int* __restrict__ sizes, int blank, int B, int K,
                                                              const int* __restrict__ pcnt, const int* __restrict__ pcls,
                                                              const float* __restrict__ plp, int* __restrict__ parent_,
                                                              int* __restrict__ label_, int* __restrict__ frame_,
                                                              int* __restrict__ tokens, int* __restrict__ offsets,
                                                              int* __restrict__ lens, float* __restrict__ scores, Extra... extra) {
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

  constexpr bool GRID = LastIs<GridArgs, Extra...>::value, STREAM = LastIs<StreamArgs, Extra...>::value;
  constexpr bool HOT = Has<HotArgs, Extra...>::value;
  constexpr bool CLM = Has<ClmArgs, Extra...>::value;
  [[maybe_unused]] const auto A = lm_args(extra...);
  [[maybe_unused]] const auto CA = clm_args(extra...);
  [[maybe_unused]] const auto H = hot_args(extra...);
  const int n = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  int size = sizes ? sizes[n] : T;
  size = size < 0 ? 0 : (size > T ? T : size);
  long fbase = (long)n * T;                            // kept list of frame t at fbase + t
  long pool = (long)n * (T + 1) * B;
  if constexpr (GRID) pool += grid_pool(extra...);
  int t0 = 0;                                          // frames before this launch's first one (a stream's consumed count)
  long rows = T;                                       // ints between two rows of tokens / offsets
  [[maybe_unused]] int* hdr = nullptr;
  if constexpr (STREAM) {
    const StreamArgs& SA = stream_args(extra...);
    hdr = (int*)(SA.state + (long)n * SA.state_stride);
    t0 = hdr[0];
    if (t0 < 0 || (long)t0 + size > SA.max_frames) {   // the chunk does not fit the pool: nothing is consumed
      if (size > 0 && tid == 0) hdr[2] = 1;
      size = 0;
      t0 = t0 < 0 ? 0 : t0;
    }
    fbase -= t0;
    pool = (long)n * (SA.max_frames + 1) * B;
    rows = SA.row_stride;
  }
  const int tend = t0 + size;
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
    if constexpr (LM) {
      LmState* L = lm_state();
      L[0].lm[0] = 0.f;
      L[0].spb[0] = A.lexicon ? -INFINITY : 0.f;
      L[0].whash[0] = kHashEmpty;
      L[0].wid[0] = -1;
#pragma unroll
      for (int m = 0; m < BEAM_LM_MAX_ORDER - 1; ++m) L[0].ctx[m][0] = A.bos;
    }
    if constexpr (CLM) {
      ClmState* L = clm_state();
      int cx[BEAM_LM_MAX_ORDER - 1];
      float bo[BEAM_LM_MAX_ORDER - 1];
#pragma unroll
      for (int m = 0; m < BEAM_LM_MAX_ORDER - 1; ++m) cx[m] = CA.bos;
      clm_backoffs(CA, cx, bo);
      L[0].lm[0] = 0.f;
#pragma unroll
      for (int m = 0; m < BEAM_LM_MAX_ORDER - 1; ++m) {
        L[0].ctx[m][0] = cx[m];
        L[0].bo[m][0] = bo[m];
      }
    }
    if constexpr (HOT) {
      HotState* HS = hot_state();
      HS[0].mh[0] = kHashEmpty;
      HS[0].done[0] = 0.f;
      HS[0].hv[0] = 0.f;
      HS[0].hsv[0] = 0.f;
      HS[0].flags[0] = 0;
      if constexpr (!LM) hot_word()[0].whash[0] = kHashEmpty;
    }
  }
  int nb = 1, cur = 0;
  if constexpr (STREAM) {
    if (t0 > 0) {                                      // a stream under way: the state that the previous feed stored
      nb = hdr[1];
      nb = nb < 0 ? 0 : (nb > B ? B : nb);
      if (tid < nb) {
        const char* sp = (const char*)hdr + kStreamHeader;
        const float* sf = (const float*)(sp + 8l * B);
        const int* si = (const int*)(sf + 3l * B);
        st[0].hash[tid] = ((const uint64_t*)sp)[tid];
        st[0].pb[tid] = sf[tid];
        st[0].pnb[tid] = sf[B + tid];
        st[0].lpc[tid] = sf[2 * B + tid];
        st[0].len[tid] = si[tid];
        st[0].last[tid] = si[B + tid];
        st[0].node[tid] = si[2 * B + tid];
        if constexpr (LM) {
          LmState* L = lm_state();
          const char* lp = sp + (long)kStreamBeamBytes * B;
          const float* lf = (const float*)(lp + 8l * B);
          const int* li = (const int*)(lf + 2l * B);
          L[0].whash[tid] = ((const uint64_t*)lp)[tid];
          L[0].lm[tid] = lf[tid];
          L[0].spb[tid] = lf[B + tid];
          L[0].wid[tid] = li[tid];
#pragma unroll
          for (int m = 0; m < BEAM_LM_MAX_ORDER - 1; ++m) L[0].ctx[m][tid] = li[(1 + m) * B + tid];
        }
        if constexpr (CLM) {
          ClmState* L = clm_state();
          const float* lf = (const float*)(sp + (long)kStreamBeamBytes * B);
          L[0].lm[tid] = lf[tid];
#pragma unroll
          for (int m = 0; m < BEAM_LM_MAX_ORDER - 1; ++m) {
            L[0].ctx[m][tid] = ((const int*)lf)[(1 + m) * B + tid];
            L[0].bo[m][tid] = lf[(BEAM_LM_MAX_ORDER + m) * B + tid];
          }
        }
        if constexpr (HOT) {
          HotState* HS = hot_state();
          const char* hp = sp + stream_hot_off(LM, B);
          const float* hf = (const float*)(hp + (LM ? 8l : 16l) * B);
          HS[0].mh[tid] = ((const uint64_t*)hp)[tid];
          if constexpr (!LM) hot_word()[0].whash[tid] = ((const uint64_t*)hp)[B + tid];
          HS[0].done[tid] = hf[tid];
          HS[0].hv[tid] = hf[B + tid];
          HS[0].hsv[tid] = hf[2 * B + tid];
          HS[0].flags[tid] = ((const int*)hf)[3 * B + tid];
        }
      }
    }
  }
  // kept list of the next frame, in registers of wave 0 (lane k holds slot k)
  int pf_cnt = 0, pf_c = 0;
  float pf_lp = 0.f;
  [[maybe_unused]] int pf_id = -1;                     // character LM: the unigram id of pf_c
  if (size > 0) {
    pf_cnt = pcnt[fbase + t0];
    if (tid < K) {
      pf_c = pcls[(fbase + t0) * BEAM_MAXK + tid];
      pf_lp = plp[(fbase + t0) * BEAM_MAXK + tid];
      if constexpr (CLM) pf_id = CA.cid[pf_c < 0 ? 0 : (pf_c >= C ? C - 1 : pf_c)];
    }
  }
  __syncthreads();

  for (int t = t0; t < tend; ++t) {
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
      // the kept classes' unigram ids, in the histogram's room: P4 zeroes it only after P2 and P3 are done with them
      if constexpr (CLM) ((int*)hist)[tid] = pf_id;
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
    if (t + 1 < tend) {
      pf_cnt = pcnt[fbase + t + 1];
      if (tid < K) {
        pf_c = pcls[(fbase + t + 1) * BEAM_MAXK + tid];
        pf_lp = plp[(fbase + t + 1) * BEAM_MAXK + tid];
        if constexpr (CLM) pf_id = CA.cid[pf_c < 0 ? 0 : (pf_c >= C ? C - 1 : pf_c)];
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
          if constexpr (HOT) {
            // hot(i+c): the space label takes the cached value; any other label probes mu+c and partial word+c together.  In
            // lexicon mode the word table's first slot is loaded before that probe, so the three loads travel together.
            const HotState& HS = hot_state()[cur];
            float hot, l = 0.f;
            if (c == H.space) {
              hot = HS.done[i] + HS.hsv[i];
              if constexpr (LM) l = lm_state()[cur].lm[i] + lm_state()[cur].spb[i];
            } else {
              uint64_t wh, wk = 0, m2, e;
              ulonglong2 w0 = {kTabEmpty, 0};
              bool lex = false;
              if constexpr (LM) {
                wh = lm_state()[cur].whash[i];
                l = lm_state()[cur].lm[i];
                lex = A.lexicon;
                wk = hash_ext(wh, c);
                if (lex) w0 = A.wtab[tab_slot(wk, A.wmask)];
              } else {
                wh = hot_word()[cur].whash[i];
              }
              const bool matched = hot_match(H, HS.mh[i], wh, c, m2, e);
              hot = HS.done[i] + (matched ? hot_v(e) : 0.f);
              if constexpr (LM) {
                // a candidate that spells no word prefix survives only inside a hot phrase
                if (lex && !matched && w0.x != wk && (w0.x == kTabEmpty || word_lookup(A, wk) == kWordAbsent)) l = -INFINITY;
              }
            }
            if constexpr (LM) s = (mass + l) + hot;
            else s = mass + hot;
          } else if constexpr (LM) {
            const LmState& LS = lm_state()[cur];
            float l = LS.lm[i];
            if (c == A.space) l += LS.spb[i];   // a word event; 0 (open mode) or -inf (lexicon mode) where it is none
            else if (A.lexicon && word_lookup(A, hash_ext(LS.whash[i], c)) == kWordAbsent) l = -INFINITY;
            s = mass + l;
          } else if constexpr (CLM) {
            // a label event: the bonus of this label after the beam's context, probed here for a new candidate only
            const ClmState& LS = clm_state()[cur];
            int cx[BEAM_LM_MAX_ORDER - 1];
            float bo[BEAM_LM_MAX_ORDER - 1];
#pragma unroll
            for (int m2 = 0; m2 < BEAM_LM_MAX_ORDER - 1; ++m2) {
              cx[m2] = LS.ctx[m2][i];
              bo[m2] = LS.bo[m2][i];
            }
            s = mass + (LS.lm[i] + clm_bonus(CA, ((const int*)hist)[k], cx, bo));
          }
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
      if constexpr (HOT) {
        const float hot = hot_state()[cur].done[i] + hot_state()[cur].hv[i];
        if constexpr (LM) cs[i * W] = (lse(npb, npnb) + lm_state()[cur].lm[i]) + hot;
        else cs[i * W] = lse(npb, npnb) + hot;
      } else if constexpr (LM) cs[i * W] = lse(npb, npnb) + lm_state()[cur].lm[i];
      else if constexpr (CLM) cs[i * W] = lse(npb, npnb) + clm_state()[cur].lm[i];
      else cs[i * W] = lse(npb, npnb);
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
        if constexpr (LM) {
          const LmState& LS = lm_state()[cur];
          LmState& LD = lm_state()[cur ^ 1];
          LD.lm[r] = LS.lm[i];
          LD.spb[r] = LS.spb[i];
          LD.whash[r] = LS.whash[i];
          LD.wid[r] = LS.wid[i];
#pragma unroll
          for (int m2 = 0; m2 < BEAM_LM_MAX_ORDER - 1; ++m2) LD.ctx[m2][r] = LS.ctx[m2][i];
        }
        if constexpr (CLM) {
          const ClmState& LS = clm_state()[cur];
          ClmState& LD = clm_state()[cur ^ 1];
          LD.lm[r] = LS.lm[i];
#pragma unroll
          for (int m2 = 0; m2 < BEAM_LM_MAX_ORDER - 1; ++m2) {
            LD.ctx[m2][r] = LS.ctx[m2][i];
            LD.bo[m2][r] = LS.bo[m2][i];
          }
        }
        if constexpr (HOT) {
          const HotState& HS = hot_state()[cur];
          HotState& HD = hot_state()[cur ^ 1];
          HD.mh[r] = HS.mh[i];
          HD.done[r] = HS.done[i];
          HD.hv[r] = HS.hv[i];
          HD.hsv[r] = HS.hsv[i];
          HD.flags[r] = HS.flags[i];
          if constexpr (!LM) hot_word()[cur ^ 1].whash[r] = hot_word()[cur].whash[i];
        }
      } else {
        const int c = kc[m - 1];
        const int id = t * B + r;
        D.pb[r] = -INFINITY;
        if constexpr (LM || HOT || CLM) D.pnb[r] = (c == S.last[i] ? S.pb[i] : score[i]) + klp[m - 1];   // the acoustic mass, as P2 formed it
        else D.pnb[r] = cs[q];
        D.lpc[r] = klp[m - 1];
        D.hash[r] = hash_ext(S.hash[i], c);
        D.len[r] = S.len[i] + 1;
        D.last[r] = c;
        D.node[r] = id;
        parent[id] = S.node[i];
        label[id] = c;
        frame[id] = t;
        [[maybe_unused]] int hflags = 0;                 // the new string's hot-word flags
        if constexpr (HOT) {
          const HotState& HS = hot_state()[cur];
          HotState& HD = hot_state()[cur ^ 1];
          uint64_t wh;
          if constexpr (LM) wh = lm_state()[cur].whash[i];
          else wh = hot_word()[cur].whash[i];
          if (c == H.space) {
            // a whole phrase is paid into done; a match that goes on past the space keeps its hash; nothing else survives a space
            const int f = HS.flags[i];
            const bool complete = f & kHotComplete, keep = (f & kHotCovered) && !complete;
            HD.mh[r] = keep ? hash_ext(HS.mh[i], c) : kHashEmpty;
            HD.done[r] = complete ? HS.done[i] + HS.hsv[i] : HS.done[i];
            HD.hv[r] = keep ? HS.hsv[i] : 0.f;
            HD.hsv[r] = 0.f;
            HD.flags[r] = 0;
            if constexpr (!LM) hot_word()[cur ^ 1].whash[r] = kHashEmpty;
          } else {
            // the probes of P2 again, then one more for mu + space, which fills the cached space values
            uint64_t m2, e;
            const bool matched = hot_match(H, HS.mh[i], wh, c, m2, e);
            const uint64_t key[1] = {hash_ext(m2, H.space)};
            uint64_t val[1];
            const bool next = hot_find<1>(H, key, matched ? 1u : 0u, val) != 0;
            const bool complete = matched && (e >> 63);
            hflags = (complete || next ? kHotCovered : 0) | (complete ? kHotComplete : 0);
            HD.mh[r] = m2;
            HD.done[r] = HS.done[i];
            HD.hv[r] = matched ? hot_v(e) : 0.f;
            HD.hsv[r] = complete ? hot_c(e) : (next ? hot_v(val[0]) : 0.f);
            HD.flags[r] = hflags;
            if constexpr (!LM) hot_word()[cur ^ 1].whash[r] = hash_ext(wh, c);
          }
        }
        if constexpr (LM) {
          const LmState& LS = lm_state()[cur];
          LmState& LD = lm_state()[cur ^ 1];
          int cx[BEAM_LM_MAX_ORDER - 1];
#pragma unroll
          for (int m2 = 0; m2 < BEAM_LM_MAX_ORDER - 1; ++m2) cx[m2] = LS.ctx[m2][i];
          if (c == A.space) {
            LD.lm[r] = LS.lm[i] + LS.spb[i];
            if (LS.whash[i] != kHashEmpty) {       // a word event: the context takes the word's id (-1: out of vocabulary)
#pragma unroll
              for (int m2 = BEAM_LM_MAX_ORDER - 2; m2 > 0; --m2) cx[m2] = cx[m2 - 1];
              cx[0] = LS.wid[i];
            }
            LD.spb[r] = A.lexicon ? -INFINITY : 0.f;
            LD.whash[r] = kHashEmpty;
            LD.wid[r] = -1;
          } else {
            const uint64_t wh = hash_ext(LS.whash[i], c);
            const int v = word_lookup(A, wh);
            const int id = v >= 0 ? v : -1;
            LD.lm[r] = LS.lm[i];
            if constexpr (HOT) {
              // an out-of-vocabulary word whose space is covered: charged hot_oov_logp, and kHotWord enters the context
              const bool cov = id < 0 && (hflags & kHotCovered);
              LD.spb[r] = cov ? lm_bonus(A, (double)H.oov_logp) : ((A.lexicon && id < 0) ? -INFINITY : word_bonus<true>(A, id, cx));
              LD.whash[r] = wh;
              LD.wid[r] = cov ? kHotWord : id;
            } else {
              LD.spb[r] = (A.lexicon && id < 0) ? -INFINITY : word_bonus<false>(A, id, cx);
              LD.whash[r] = wh;
              LD.wid[r] = id;
            }
          }
#pragma unroll
          for (int m2 = 0; m2 < BEAM_LM_MAX_ORDER - 1; ++m2) LD.ctx[m2][r] = cx[m2];
        }
        if constexpr (CLM) {
          // the candidate's total less its acoustic mass is not its lm bit for bit, so the bonus is formed again as P2 formed it
          const ClmState& LS = clm_state()[cur];
          ClmState& LD = clm_state()[cur ^ 1];
          int cx[BEAM_LM_MAX_ORDER - 1];
          float bo[BEAM_LM_MAX_ORDER - 1];
#pragma unroll
          for (int m2 = 0; m2 < BEAM_LM_MAX_ORDER - 1; ++m2) {
            cx[m2] = LS.ctx[m2][i];
            bo[m2] = LS.bo[m2][i];
          }
          const int w = CA.cid[c];
          LD.lm[r] = LS.lm[i] + clm_bonus(CA, w, cx, bo);
#pragma unroll
          for (int m2 = BEAM_LM_MAX_ORDER - 2; m2 > 0; --m2) cx[m2] = cx[m2 - 1];
          cx[0] = w;
          clm_backoffs(CA, cx, bo);
#pragma unroll
          for (int m2 = 0; m2 < BEAM_LM_MAX_ORDER - 1; ++m2) {
            LD.ctx[m2][r] = cx[m2];
            LD.bo[m2][r] = bo[m2];
          }
        }
      }
    }
    if (tid < nk) kidx[kc[tid]] = -1;
    nb = ns;
    cur ^= 1;
    __syncthreads();
  }

  if constexpr (STREAM) {
    if (size > 0) {                                    // the state after this chunk, for the next feed
      const BeamState& E = st[cur];
      if (tid < nb) {
        char* sp = (char*)hdr + kStreamHeader;
        float* sf = (float*)(sp + 8l * B);
        int* si = (int*)(sf + 3l * B);
        ((uint64_t*)sp)[tid] = E.hash[tid];
        sf[tid] = E.pb[tid];
        sf[B + tid] = E.pnb[tid];
        sf[2 * B + tid] = E.lpc[tid];
        si[tid] = E.len[tid];
        si[B + tid] = E.last[tid];
        si[2 * B + tid] = E.node[tid];
        if constexpr (LM) {
          const LmState& LE = lm_state()[cur];
          char* lp = sp + (long)kStreamBeamBytes * B;
          float* lf = (float*)(lp + 8l * B);
          int* li = (int*)(lf + 2l * B);
          ((uint64_t*)lp)[tid] = LE.whash[tid];
          lf[tid] = LE.lm[tid];
          lf[B + tid] = LE.spb[tid];
          li[tid] = LE.wid[tid];
#pragma unroll
          for (int m = 0; m < BEAM_LM_MAX_ORDER - 1; ++m) li[(1 + m) * B + tid] = LE.ctx[m][tid];
        }
        if constexpr (CLM) {
          const ClmState& LE = clm_state()[cur];
          float* lf = (float*)(sp + (long)kStreamBeamBytes * B);
          lf[tid] = LE.lm[tid];
#pragma unroll
          for (int m = 0; m < BEAM_LM_MAX_ORDER - 1; ++m) {
            ((int*)lf)[(1 + m) * B + tid] = LE.ctx[m][tid];
            lf[(BEAM_LM_MAX_ORDER + m) * B + tid] = LE.bo[m][tid];
          }
        }
        if constexpr (HOT) {
          const HotState& HE = hot_state()[cur];
          char* hp = sp + stream_hot_off(LM, B);
          float* hf = (float*)(hp + (LM ? 8l : 16l) * B);
          ((uint64_t*)hp)[tid] = HE.mh[tid];
          if constexpr (!LM) ((uint64_t*)hp)[B + tid] = hot_word()[cur].whash[tid];
          hf[tid] = HE.done[tid];
          hf[B + tid] = HE.hv[tid];
          hf[2 * B + tid] = HE.hsv[tid];
          ((int*)hf)[3 * B + tid] = HE.flags[tid];
        }
      }
      if (tid == 0) {
        hdr[0] = tend;
        hdr[1] = nb;
      }
    }
    if (!tokens) return;                               // a feed without the output stage
  }
  // ---- output: one thread per rank walks the parent links
  __threadfence();
  __syncthreads();
  __threadfence();
  const BeamState& S = st[cur];
  int orank = tid;
  [[maybe_unused]] float* acoustic = nullptr;
  if constexpr (LM) acoustic = A.acoustic;
  else if constexpr (HOT) acoustic = H.acoustic;
  else if constexpr (CLM) acoustic = CA.acoustic;
  if constexpr (HOT) {
    // end of utterance with hot words: hot_end pays a match that is a whole phrase and nothing for an unfinished one; with an
    // LM the end is covered only by a whole phrase, so a hot word cut short is out of vocabulary again.  Re-ranked by the total.
    const HotState& HS = hot_state()[cur];
    float tot = 0.f;
    if (tid < nb) {
      const float ac = lse(S.pb[tid], S.pnb[tid]);
      const bool complete = HS.flags[tid] & kHotComplete;
      const float hot_end = complete ? HS.done[tid] + HS.hsv[tid] : HS.done[tid];
      if constexpr (LM) {
        const LmState& LS = lm_state()[cur];
        float l = LS.lm[tid];
        if (LS.whash[tid] != kHashEmpty) {
          if (LS.wid[tid] == kHotWord) l += complete ? LS.spb[tid] : lm_bonus(A, kOovScore);
          else l += LS.spb[tid] == -INFINITY ? lm_bonus(A, kOovScore) : LS.spb[tid];
        }
        tot = (ac + l) + hot_end;
      } else {
        tot = ac + hot_end;
      }
      score[tid] = tot;
      stay_pb[tid] = ac;
    }
    __syncthreads();
    if (tid < nb) {
      orank = 0;
      for (int s = 0; s < nb; ++s) orank += score[s] > tot || (score[s] == tot && s < tid);
    }
  } else if constexpr (LM) {
    // end of utterance: a beam that ends inside a word gets that word's bonus too (a mere prefix counts as out of vocabulary in
    // lexicon mode); the beams are re-ranked by the total, ties to the earlier rank
    const LmState& LS = lm_state()[cur];
    float tot = 0.f;
    if (tid < nb) {
      const float ac = lse(S.pb[tid], S.pnb[tid]);
      float l = LS.lm[tid];
      if (LS.whash[tid] != kHashEmpty) l += LS.spb[tid] == -INFINITY ? lm_bonus(A, kOovScore) : LS.spb[tid];
      tot = ac + l;
      score[tid] = tot;
      stay_pb[tid] = ac;
    }
    __syncthreads();
    if (tid < nb) {
      orank = 0;
      for (int s = 0; s < nb; ++s) orank += score[s] > tot || (score[s] == tot && s < tid);
    }
  }
  if constexpr (CLM) {
    // no end-of-utterance term and no re-rank: the ranks are the last selection's
    if (tid < nb) {
      const float ac = lse(S.pb[tid], S.pnb[tid]);
      score[tid] = ac + clm_state()[cur].lm[tid];
      stay_pb[tid] = ac;
    }
  }
  // every rank writes its row; in a grid only rank 0 does (thread 0 where no beam is alive), at row (g, n)
  bool emit = GRID ? orank == 0 : true;
  if constexpr (STREAM) emit = orank < stream_args(extra...).out_ranks;   // a stream writes its best out_ranks beams only
  if (tid < B && emit) {
    long o = GRID ? (long)blockIdx.y * gridDim.x + n : (long)n * B + orank;
    if constexpr (STREAM) o = (long)n * stream_args(extra...).out_ranks + orank;
    if (tid < nb) {
      const int len = S.len[tid];
      int node = S.node[tid];
      int* tok = tokens + o * rows;
      int* off = GRID && !offsets ? nullptr : offsets + o * rows;
      for (int pos = len - 1; pos >= 0 && node >= 0; --pos) {
        if constexpr (STREAM) {
          if (pos >= rows) {                           // a row shorter than the string: never written past
            node = parent[node];
            continue;
          }
        }
        tok[pos] = label[node];
        if (!GRID || off) off[pos] = frame[node];
        node = parent[node];
      }
      lens[o] = len;
      if constexpr (LM || HOT || CLM) {
        scores[o] = -score[tid] + 0.f;
        if (acoustic) acoustic[o] = -stay_pb[tid] + 0.f;
      } else {
        scores[o] = -lse(S.pb[tid], S.pnb[tid]) + 0.f;
      }
    } else {
      lens[o] = 0;
      scores[o] = INFINITY;
      if constexpr (LM || HOT || CLM) {
        if (acoustic) acoustic[o] = INFINITY;
      }
    }
  }
}

long align256(long b) { return (b + 255) / 256 * 256; }

struct WsLayout {
  long cnt, cls, lp, parent, label, frame, total, pool;   // byte offsets; pool = bytes of one point's node pool, per array
};

// the kept lists once, then G node pools per array (G = 1 outside a grid)
WsLayout ws_layout(int N, int T, int B, int G = 1) {
  WsLayout L;
  const long frames = (long)N * T, nodes = (long)N * (T + 1) * B;
  L.pool = align256(nodes * 4);
  L.cnt = 0;
  L.cls = L.cnt + align256(frames * 4);
  L.lp = L.cls + align256(frames * BEAM_MAXK * 4);
  L.parent = L.lp + align256(frames * BEAM_MAXK * 4);
  L.label = L.parent + G * L.pool;
  L.frame = L.label + G * L.pool;
  L.total = L.frame + G * L.pool;
  return L;
}

int beam_decode(const float* x, long stride_n, long stride_t, int N, int T, int C, const int* sizes, int blank, int B,
                int cutoff_top_n, float cutoff_prob, int* tokens, int* offsets, int* lens, float* scores, void* ws, hipStream_t st,
                const LmArgs* lm, int G = 1, const float* alphas = nullptr, const float* betas = nullptr,
                const HotArgs* hot = nullptr, const ClmArgs* clm = nullptr);

// A stream session's buffer: the states, then the node pool's three arrays
struct StreamLayout {
  long state_stride, parent, label, frame, total;   // bytes
};

constexpr int kStreamFlagLm = 1, kStreamFlagHot = 2;   // the flag word of the ds2_beam_stream_* size queries and reset
constexpr int kStreamFlagClm = 4;                      // with kStreamFlagLm and without hot words: the model scores characters
// the flag words that name a form of the search: 0 .. 3, and 5 (the character LM's state has the size of the word LM's)
bool stream_flags_ok(int flags) { return (flags >= 0 && flags <= 3) || flags == (kStreamFlagLm | kStreamFlagClm); }

StreamLayout stream_layout(int N, int B, int max_frames, int flags) {
  StreamLayout L;
  const bool lm = flags & kStreamFlagLm;
  long beams = (long)B * (kStreamBeamBytes + (lm ? kStreamLmBytes : 0));
  if (flags & kStreamFlagHot) beams = stream_hot_off(lm, B) + (long)B * (kStreamHotBytes + (lm ? 0 : 8));
  L.state_stride = align256(kStreamHeader + beams);
  const long pool = align256((long)N * ((long)max_frames + 1) * B * 4);
  L.parent = (long)N * L.state_stride;
  L.label = L.parent + pool;
  L.frame = L.label + pool;
  L.total = L.frame + pool;
  return L;
}

// the kept lists of one chunk
WsLayout stream_ws_layout(int N, int Tc) {
  WsLayout L = {};
  const long frames = (long)N * Tc;
  L.cls = align256(frames * 4);
  L.lp = L.cls + align256(frames * BEAM_MAXK * 4);
  L.total = L.lp + align256(frames * BEAM_MAXK * 4);
  return L;
}

__global__ void k_beam_stream_reset(char* state, long state_stride, int N, const int* __restrict__ mask) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n < N && (!mask || mask[n])) *(int4*)(state + (long)n * state_stride) = make_int4(0, 0, 0, 0);
}

int beam_stream_feed(const float* x, long stride_n, long stride_t, int N, int Tc, int C, const int* sizes, int blank, int B,
                     int cutoff_top_n, float cutoff_prob, void* state, int max_frames, int* tokens, int* offsets, long row_stride,
                     int out_ranks, int* lens, float* scores, void* ws, hipStream_t st, const LmArgs* lm,
                     const HotArgs* hot = nullptr, const ClmArgs* clm = nullptr);

// the checks and the fields of the hot-word entry points
int hot_args_from(HotArgs& H, int C, int blank, int space, const void* hot_table, long hot_slots, float oov_logp, float* acoustic) {
  DS2_REQUIRE(C > 0 && space >= 0 && space < C && space != blank, DS2_ERR_ARG);
  DS2_REQUIRE(hot_table && hot_slots >= 2 && hot_slots <= (1l << 31) && (hot_slots & (hot_slots - 1)) == 0, DS2_ERR_ARG);
  DS2_REQUIRE(oov_logp == oov_logp && oov_logp > -INFINITY && oov_logp < INFINITY, DS2_ERR_ARG);
  DS2_REQUIRE(((uintptr_t)hot_table & 15) == 0, DS2_ERR_ALIGN);
  H.htab = (const ulonglong2*)hot_table;
  H.hmask = (unsigned)(hot_slots - 1);
  H.space = space;
  H.oov_logp = oov_logp;
  H.acoustic = acoustic;
  return 0;
}

// the checks and the fields of the language-model entry points (the grid form passes alpha = beta = 0: its points carry them)
int lm_args_from(LmArgs& A, int C, int blank, int space, const void* word_table, long word_slots, const void* ngram_table,
                 long ngram_slots, int order, int bos, float alpha, float beta, int lexicon, float* acoustic) {
  DS2_REQUIRE(C > 0 && space >= 0 && space < C && space != blank, DS2_ERR_ARG);
  DS2_REQUIRE(order >= 1 && order <= BEAM_LM_MAX_ORDER && bos >= 0, DS2_ERR_ARG);
  DS2_REQUIRE(word_table && ngram_table, DS2_ERR_ARG);
  DS2_REQUIRE(word_slots >= 2 && word_slots <= (1l << 31) && (word_slots & (word_slots - 1)) == 0, DS2_ERR_ARG);
  DS2_REQUIRE(ngram_slots >= 2 && ngram_slots <= (1l << 31) && (ngram_slots & (ngram_slots - 1)) == 0, DS2_ERR_ARG);
  DS2_REQUIRE((((uintptr_t)word_table | (uintptr_t)ngram_table) & 15) == 0, DS2_ERR_ALIGN);
  A.wtab = (const ulonglong2*)word_table;
  A.gtab = (const ulonglong2*)ngram_table;
  A.wmask = (unsigned)(word_slots - 1);
  A.gmask = (unsigned)(ngram_slots - 1);
  A.space = space;
  A.order = order;
  A.bos = bos;
  A.lexicon = lexicon != 0;
  A.alpha = alpha;
  A.beta = beta;
  A.acoustic = acoustic;
  return 0;
}

// the checks and the fields of the character-LM entry points (the grid form passes alpha = beta = 0: its points carry them)
int clm_args_from(ClmArgs& A, int C, const int* cid, const void* ngram_table, long ngram_slots, int order, int bos, float alpha,
                  float beta, float* acoustic) {
  DS2_REQUIRE(C > 0 && cid && ngram_table, DS2_ERR_ARG);
  DS2_REQUIRE(order >= 1 && order <= BEAM_LM_MAX_ORDER && bos >= 0, DS2_ERR_ARG);
  DS2_REQUIRE(ngram_slots >= 2 && ngram_slots <= (1l << 31) && (ngram_slots & (ngram_slots - 1)) == 0, DS2_ERR_ARG);
  DS2_REQUIRE(((uintptr_t)ngram_table & 15) == 0 && ((uintptr_t)cid & 3) == 0, DS2_ERR_ALIGN);
  A.cid = cid;
  A.gtab = (const ulonglong2*)ngram_table;
  A.gmask = (unsigned)(ngram_slots - 1);
  A.order = order;
  A.bos = bos;
  A.alpha = alpha;
  A.beta = beta;
  A.acoustic = acoustic;
  return 0;
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
  return beam_decode(x, stride_n, stride_t, N, T, C, sizes, blank, B, cutoff_top_n, cutoff_prob, tokens, offsets, lens, scores, ws,
                     (hipStream_t)st_, nullptr);
}

// The same search with a word n-gram language model (DESIGN.md "ds2_beam", language model).  space: the label that ends a word.
// word_table / ngram_table: the open-addressing tables of lm.py, [slots][2] 64-bit words, slots a power of two, 16-byte aligned.
// order 1 .. 5; bos: the id of <s>; lexicon != 0 drops candidates that spell no word prefix.  scores = -(acoustic + lm), the
// quantity that ranks the beams; acoustic (may be null): -lse(pb, pnb) of the same ranks.  ws as for ds2_beam_decode.
int ds2_beam_decode_lm(const float* x, long stride_n, long stride_t, int N, int T, int C, const int* sizes, int blank, int B,
                       int cutoff_top_n, float cutoff_prob, int space, const void* word_table, long word_slots,
                       const void* ngram_table, long ngram_slots, int order, int bos, float alpha, float beta, int lexicon,
                       int* tokens, int* offsets, int* lens, float* scores, float* acoustic, void* ws, ds2_stream_t st_) {
  LmArgs A;
  const int rc = lm_args_from(A, C, blank, space, word_table, word_slots, ngram_table, ngram_slots, order, bos, alpha, beta, lexicon,
                              acoustic);
  if (rc) return rc;
  return beam_decode(x, stride_n, stride_t, N, T, C, sizes, blank, B, cutoff_top_n, cutoff_prob, tokens, offsets, lens, scores, ws,
                     (hipStream_t)st_, &A);
}

// flags: bit 0 a language model, bit 1 hot words (0 and 1 are the former values of this argument), bit 2 the language model
// scores characters (only as 5: with bit 0, without bit 1); any other word gives 0
long ds2_beam_stream_bytes(int N, int B, int max_frames, int flags) {
  if (N <= 0 || B <= 0 || max_frames <= 0 || !stream_flags_ok(flags)) return 0;
  return stream_layout(N, B, max_frames, flags).total;
}

// bytes between two streams' states at the front of a session's buffer
long ds2_beam_stream_state_stride(int B, int flags) {
  if (B <= 0 || !stream_flags_ok(flags)) return 0;
  return stream_layout(1, B, 1, flags).state_stride;
}

long ds2_beam_stream_ws_bytes(int N, int Tc) {
  if (N <= 0 || Tc <= 0) return 0;
  return stream_ws_layout(N, Tc).total;
}

// state: the session's buffer, ds2_beam_stream_bytes(N, B, max_frames, flags) bytes, 256-byte aligned.  mask: [N] device int32, a
// stream with a non-zero entry starts again from the empty beam (null = every stream); the others are untouched.  A new buffer is
// reset as a whole before its first feed.
int ds2_beam_stream_reset(void* state, int N, int B, int max_frames, int flags, const int* mask, ds2_stream_t st_) {
  DS2_REQUIRE(state && N > 0 && B >= 1 && B <= BEAM_MAXB && max_frames > 0 && stream_flags_ok(flags), DS2_ERR_ARG);
  DS2_REQUIRE(((uintptr_t)state & 255) == 0, DS2_ERR_ALIGN);
  const StreamLayout L = stream_layout(N, B, max_frames, flags);
  hipLaunchKernelGGL(k_beam_stream_reset, dim3((unsigned)((N + 63) / 64)), dim3(64), 0, (hipStream_t)st_, (char*)state,
                     L.state_stride, N, mask);
  DS2_CHECK_LAUNCH();
  return 0;
}

// One chunk of every stream: x is the chunk (N, Tc, C) with ds2_beam_decode's strides, sizes [N] (device int32, null = Tc) the
// frames of it that each stream takes, 0 leaving that stream as it is.  A stream whose consumed count would pass max_frames
// takes nothing and has its overflow flag (the third int of its state) set.  tokens / offsets / lens / scores are either all null
// (no output stage) or all given: then rows (n, b), b < out_ranks <= B, of tokens / offsets, row_stride ints apart with row_stride
// >= the largest consumed count, lens [N][out_ranks] and scores [N][out_ranks] are the best out_ranks beams that ds2_beam_decode
// gives on the frames consumed so far, bit for bit, and the state is left as the feed left it.  Tc == 0 (x, sizes and ws unused) only runs the output stage.
// ws: ds2_beam_stream_ws_bytes(N, Tc) bytes, 256-byte aligned.  B, max_frames, blank and the cutoffs are the session's: the same
// in every call on one state buffer.
int ds2_beam_stream_feed(const float* x, long stride_n, long stride_t, int N, int Tc, int C, const int* sizes, int blank, int B,
                         int cutoff_top_n, float cutoff_prob, void* state, int max_frames, int* tokens, int* offsets,
                         long row_stride, int out_ranks, int* lens, float* scores, void* ws, ds2_stream_t st_) {
  return beam_stream_feed(x, stride_n, stride_t, N, Tc, C, sizes, blank, B, cutoff_top_n, cutoff_prob, state, max_frames, tokens,
                          offsets, row_stride, out_ranks, lens, scores, ws, (hipStream_t)st_, nullptr);
}

// ds2_beam_stream_feed with the language model of ds2_beam_decode_lm (the same tables and weights in every call on one state
// buffer, which was sized with lm = 1).  The output stage includes the end-of-utterance bonus and re-rank, which read the state
// and leave it unchanged; acoustic [N][out_ranks] may be null.
int ds2_beam_stream_feed_lm(const float* x, long stride_n, long stride_t, int N, int Tc, int C, const int* sizes, int blank, int B,
                            int cutoff_top_n, float cutoff_prob, int space, const void* word_table, long word_slots,
                            const void* ngram_table, long ngram_slots, int order, int bos, float alpha, float beta, int lexicon,
                            void* state, int max_frames, int* tokens, int* offsets, long row_stride, int out_ranks, int* lens,
                            float* scores, float* acoustic, void* ws, ds2_stream_t st_) {
  LmArgs A;
  const int rc = lm_args_from(A, C, blank, space, word_table, word_slots, ngram_table, ngram_slots, order, bos, alpha, beta, lexicon,
                              acoustic);
  if (rc) return rc;
  return beam_stream_feed(x, stride_n, stride_t, N, Tc, C, sizes, blank, B, cutoff_top_n, cutoff_prob, state, max_frames, tokens,
                          offsets, row_stride, out_ranks, lens, scores, ws, (hipStream_t)st_, &A);
}

// ds2_beam_decode with hot words (DESIGN.md "ds2_beam", hot words).  space: the label that ends a word; hot_table: the
// open-addressing table of hotwords.py, [hot_slots][2] 64-bit words, hot_slots a power of two, 16-byte aligned.  scores =
// -(log p + hot_end), the quantity that ranks the beams; acoustic (may be null): -lse(pb, pnb) of the same ranks.
int ds2_beam_decode_hot(const float* x, long stride_n, long stride_t, int N, int T, int C, const int* sizes, int blank, int B,
                        int cutoff_top_n, float cutoff_prob, int space, const void* hot_table, long hot_slots, int* tokens,
                        int* offsets, int* lens, float* scores, float* acoustic, void* ws, ds2_stream_t st_) {
  HotArgs H;
  const int rc = hot_args_from(H, C, blank, space, hot_table, hot_slots, 0.f, acoustic);
  if (rc) return rc;
  return beam_decode(x, stride_n, stride_t, N, T, C, sizes, blank, B, cutoff_top_n, cutoff_prob, tokens, offsets, lens, scores, ws,
                     (hipStream_t)st_, nullptr, 1, nullptr, nullptr, &H);
}

// ds2_beam_decode_lm with hot words.  hot_oov_logp: ln P of a word event whose word is out of vocabulary but covered by a hot
// phrase.  scores = -((log p + lm) + hot_end).
int ds2_beam_decode_lm_hot(const float* x, long stride_n, long stride_t, int N, int T, int C, const int* sizes, int blank, int B,
                           int cutoff_top_n, float cutoff_prob, int space, const void* word_table, long word_slots,
                           const void* ngram_table, long ngram_slots, int order, int bos, float alpha, float beta, int lexicon,
                           const void* hot_table, long hot_slots, float hot_oov_logp, int* tokens, int* offsets, int* lens,
                           float* scores, float* acoustic, void* ws, ds2_stream_t st_) {
  LmArgs A;
  int rc = lm_args_from(A, C, blank, space, word_table, word_slots, ngram_table, ngram_slots, order, bos, alpha, beta, lexicon,
                        acoustic);
  if (rc) return rc;
  HotArgs H;
  rc = hot_args_from(H, C, blank, space, hot_table, hot_slots, hot_oov_logp, nullptr);
  if (rc) return rc;
  return beam_decode(x, stride_n, stride_t, N, T, C, sizes, blank, B, cutoff_top_n, cutoff_prob, tokens, offsets, lens, scores, ws,
                     (hipStream_t)st_, &A, 1, nullptr, nullptr, &H);
}

// ds2_beam_stream_feed with hot words (the same table in every call on one state buffer, which was sized with flags = 2).  The
// output stage includes hot_end and the re-rank, which read the state and leave it unchanged; acoustic [N][out_ranks] may be null.
int ds2_beam_stream_feed_hot(const float* x, long stride_n, long stride_t, int N, int Tc, int C, const int* sizes, int blank, int B,
                             int cutoff_top_n, float cutoff_prob, int space, const void* hot_table, long hot_slots, void* state,
                             int max_frames, int* tokens, int* offsets, long row_stride, int out_ranks, int* lens, float* scores,
                             float* acoustic, void* ws, ds2_stream_t st_) {
  HotArgs H;
  const int rc = hot_args_from(H, C, blank, space, hot_table, hot_slots, 0.f, acoustic);
  if (rc) return rc;
  return beam_stream_feed(x, stride_n, stride_t, N, Tc, C, sizes, blank, B, cutoff_top_n, cutoff_prob, state, max_frames, tokens,
                          offsets, row_stride, out_ranks, lens, scores, ws, (hipStream_t)st_, nullptr, &H);
}

// ds2_beam_stream_feed_lm with hot words (state buffer sized with flags = 3).
int ds2_beam_stream_feed_lm_hot(const float* x, long stride_n, long stride_t, int N, int Tc, int C, const int* sizes, int blank,
                                int B, int cutoff_top_n, float cutoff_prob, int space, const void* word_table, long word_slots,
                                const void* ngram_table, long ngram_slots, int order, int bos, float alpha, float beta, int lexicon,
                                const void* hot_table, long hot_slots, float hot_oov_logp, void* state, int max_frames, int* tokens,
                                int* offsets, long row_stride, int out_ranks, int* lens, float* scores, float* acoustic, void* ws,
                                ds2_stream_t st_) {
  LmArgs A;
  int rc = lm_args_from(A, C, blank, space, word_table, word_slots, ngram_table, ngram_slots, order, bos, alpha, beta, lexicon,
                        acoustic);
  if (rc) return rc;
  HotArgs H;
  rc = hot_args_from(H, C, blank, space, hot_table, hot_slots, hot_oov_logp, nullptr);
  if (rc) return rc;
  return beam_stream_feed(x, stride_n, stride_t, N, Tc, C, sizes, blank, B, cutoff_top_n, cutoff_prob, state, max_frames, tokens,
                          offsets, row_stride, out_ranks, lens, scores, ws, (hipStream_t)st_, &A, &H);
}

long ds2_beam_grid_ws_bytes(int G, int N, int T, int B) {
  if (G <= 0 || N <= 0 || T <= 0 || B <= 0) return 0;
  return ws_layout(N, T, B, G).total;
}

// ds2_beam_decode_lm for G points (alphas[g], betas[g]) at once: the frames are pruned once, then G x N workgroups search.  Of
// every (point, sample) only the top beam after the end-of-utterance re-rank is written: tokens / offsets [G][N][T] (offsets may
// be null), lens / scores / acoustic [G][N] (acoustic may be null).  Row (g, n) equals rank 0 of sample n of ds2_beam_decode_lm
// with alpha = alphas[g], beta = betas[g], bit for bit.  ws: ds2_beam_grid_ws_bytes(G, N, T, B) bytes, 256-byte aligned.
int ds2_beam_decode_lm_grid(const float* x, long stride_n, long stride_t, int N, int T, int C, const int* sizes, int blank, int B,
                            int cutoff_top_n, float cutoff_prob, int space, const void* word_table, long word_slots,
                            const void* ngram_table, long ngram_slots, int order, int bos, int lexicon, int G, const float* alphas,
                            const float* betas, int* tokens, int* offsets, int* lens, float* scores, float* acoustic, void* ws,
                            ds2_stream_t st_) {
  DS2_REQUIRE(G >= 1 && G <= BEAM_MAX_POINTS && alphas && betas, DS2_ERR_ARG);
  LmArgs A;
  const int rc = lm_args_from(A, C, blank, space, word_table, word_slots, ngram_table, ngram_slots, order, bos, 0.f, 0.f, lexicon,
                              acoustic);
  if (rc) return rc;
  return beam_decode(x, stride_n, stride_t, N, T, C, sizes, blank, B, cutoff_top_n, cutoff_prob, tokens, offsets, lens, scores, ws,
                     (hipStream_t)st_, &A, G, alphas, betas);
}

// The search with a character n-gram language model (DESIGN.md "ds2_beam", character language model): every label is an event
// of the model.  cid: [C] device int32, the unigram id of every class, -1 where the file has none (the blank's entry is not
// read); ngram_table as for ds2_beam_decode_lm; order 1 .. 5; bos: the id of <s>.  No word table, no lexicon, no end-of-utterance
// term: scores = -(acoustic + lm) of the last selection's ranks; acoustic (may be null): -lse(pb, pnb) of the same ranks.
int ds2_beam_decode_clm(const float* x, long stride_n, long stride_t, int N, int T, int C, const int* sizes, int blank, int B,
                        int cutoff_top_n, float cutoff_prob, const int* cid, const void* ngram_table, long ngram_slots, int order,
                        int bos, float alpha, float beta, int* tokens, int* offsets, int* lens, float* scores, float* acoustic,
                        void* ws, ds2_stream_t st_) {
  ClmArgs A;
  const int rc = clm_args_from(A, C, cid, ngram_table, ngram_slots, order, bos, alpha, beta, acoustic);
  if (rc) return rc;
  return beam_decode(x, stride_n, stride_t, N, T, C, sizes, blank, B, cutoff_top_n, cutoff_prob, tokens, offsets, lens, scores, ws,
                     (hipStream_t)st_, nullptr, 1, nullptr, nullptr, nullptr, &A);
}

// ds2_beam_stream_feed with the character language model of ds2_beam_decode_clm (the same ids, table and weights in every call on
// one state buffer, which was sized with flags = 5).  acoustic [N][out_ranks] may be null.
int ds2_beam_stream_feed_clm(const float* x, long stride_n, long stride_t, int N, int Tc, int C, const int* sizes, int blank, int B,
                             int cutoff_top_n, float cutoff_prob, const int* cid, const void* ngram_table, long ngram_slots,
                             int order, int bos, float alpha, float beta, void* state, int max_frames, int* tokens, int* offsets,
                             long row_stride, int out_ranks, int* lens, float* scores, float* acoustic, void* ws, ds2_stream_t st_) {
  ClmArgs A;
  const int rc = clm_args_from(A, C, cid, ngram_table, ngram_slots, order, bos, alpha, beta, acoustic);
  if (rc) return rc;
  return beam_stream_feed(x, stride_n, stride_t, N, Tc, C, sizes, blank, B, cutoff_top_n, cutoff_prob, state, max_frames, tokens,
                          offsets, row_stride, out_ranks, lens, scores, ws, (hipStream_t)st_, nullptr, nullptr, &A);
}

// ds2_beam_decode_clm for G points (alphas[g], betas[g]) at once, as ds2_beam_decode_lm_grid: outputs of every (point, sample)'s
// top beam, row (g, n) equal to rank 0 of sample n of ds2_beam_decode_clm at that point bit for bit.  ws:
// ds2_beam_grid_ws_bytes(G, N, T, B) bytes.
int ds2_beam_decode_clm_grid(const float* x, long stride_n, long stride_t, int N, int T, int C, const int* sizes, int blank, int B,
                             int cutoff_top_n, float cutoff_prob, const int* cid, const void* ngram_table, long ngram_slots,
                             int order, int bos, int G, const float* alphas, const float* betas, int* tokens, int* offsets,
                             int* lens, float* scores, float* acoustic, void* ws, ds2_stream_t st_) {
  DS2_REQUIRE(G >= 1 && G <= BEAM_MAX_POINTS && alphas && betas, DS2_ERR_ARG);
  ClmArgs A;
  const int rc = clm_args_from(A, C, cid, ngram_table, ngram_slots, order, bos, 0.f, 0.f, acoustic);
  if (rc) return rc;
  return beam_decode(x, stride_n, stride_t, N, T, C, sizes, blank, B, cutoff_top_n, cutoff_prob, tokens, offsets, lens, scores, ws,
                     (hipStream_t)st_, nullptr, G, alphas, betas, nullptr, &A);
}

}  // extern "C"

namespace {

// the sixteen leading arguments of k_beam_search, and where it is launched
struct SearchArgs {
  dim3 grid;
  hipStream_t st;
  int T, C, blank, B, K;
  const int* sizes;
  float* plp;
  int *pcnt, *pcls, *parent, *label, *frame, *tokens, *offsets, *lens;
  float* scores;
};

// What the one-shot and the resumable search share: the checks of their common arguments, K, the kept lists' place in ws (L is
// ws_layout's or stream_ws_layout's) and the launch that fills them, none for T == 0 (min_T == 0: the resumable form allows it).
int beam_prune(SearchArgs& a, const float* x, long stride_n, long stride_t, int N, int T, int min_T, int C, const int* sizes,
               int blank, int B, int cutoff_top_n, float cutoff_prob, void* ws, const WsLayout& L, hipStream_t st) {
  DS2_REQUIRE(N > 0 && T >= min_T && C > 0 && C <= BEAM_MAXC && blank >= 0 && blank < C, DS2_ERR_ARG);
  DS2_REQUIRE(B >= 1 && B <= BEAM_MAXB && cutoff_top_n >= 1, DS2_ERR_ARG);
  const int K = cutoff_top_n < C ? cutoff_top_n : C;
  DS2_REQUIRE(K <= BEAM_MAXK, DS2_ERR_ARG);
  char* w = (char*)ws;
  a = {dim3(N), st, T, C, blank, B, K, sizes, (float*)(w + L.lp), (int*)(w + L.cnt), (int*)(w + L.cls)};
  if (T == 0) return 0;
  const int use_cut = cutoff_prob < 1.0f;
  const long frames = (long)N * T;
  hipLaunchKernelGGL(k_beam_prune, dim3((unsigned)((frames + 3) / 4)), dim3(256), 0, st, x, stride_n, stride_t, N, T, C, sizes, K,
                     use_cut, (double)cutoff_prob, a.pcnt, a.pcls, a.plp);
  DS2_CHECK_LAUNCH();
  return 0;
}

template <bool LM, class... Extra>
void launch_search(const SearchArgs& a, const Extra&... extra) {
  hipLaunchKernelGGL((k_beam_search<LM, Extra...>), a.grid, dim3(BEAM_THREADS), 0, a.st, a.T, a.C, a.sizes, a.blank, a.B, a.K, a.pcnt,
                     a.pcls, a.plp, a.parent, a.label, a.frame, a.tokens, a.offsets, a.lens, a.scores, extra...);
}

// The search with the language model and the hot words that are given.  tail: nothing, or the StreamArgs.  grid: null, or the points
// of ds2_beam_decode_lm_grid, which has a language model, no hot words and no tail.
template <class... Tail>
void launch_search_with(const SearchArgs& a, const LmArgs* lm, const HotArgs* hot, const GridArgs* grid, const ClmArgs* clm,
                        const Tail&... tail) {
  if (clm) {           // the character LM: alone, with the points of a grid, or with the tail
    if constexpr (sizeof...(Tail) == 0) grid ? launch_search<false>(a, *clm, *grid) : launch_search<false>(a, *clm);
    else launch_search<false>(a, *clm, tail...);
  } else if (hot)
    lm ? launch_search<true>(a, *lm, *hot, tail...) : launch_search<false>(a, *hot, tail...);
  else if (grid) {
    if constexpr (sizeof...(Tail) == 0) launch_search<true>(a, *lm, *grid);
  } else
    lm ? launch_search<true>(a, *lm, tail...) : launch_search<false>(a, tail...);
}

int beam_decode(const float* x, long stride_n, long stride_t, int N, int T, int C, const int* sizes, int blank, int B,
                int cutoff_top_n, float cutoff_prob, int* tokens, int* offsets, int* lens, float* scores, void* ws, hipStream_t st,
                const LmArgs* lm, int G, const float* alphas, const float* betas, const HotArgs* hot, const ClmArgs* clm) {
  DS2_REQUIRE(x && tokens && (offsets || alphas) && lens && scores && ws, DS2_ERR_ARG);
  DS2_REQUIRE(((uintptr_t)ws & 255) == 0, DS2_ERR_ALIGN);
  const WsLayout L = ws_layout(N, T, B, G);
  SearchArgs a;
  const int rc = beam_prune(a, x, stride_n, stride_t, N, T, 1, C, sizes, blank, B, cutoff_top_n, cutoff_prob, ws, L, st);
  if (rc) return rc;
  char* w = (char*)ws;
  a.parent = (int*)(w + L.parent), a.label = (int*)(w + L.label), a.frame = (int*)(w + L.frame);
  a.tokens = tokens, a.offsets = offsets, a.lens = lens, a.scores = scores;
  const GridArgs grid = {alphas, betas, L.pool / 4};
  a.grid.y = G;      // the grid form: G x N workgroups
  launch_search_with(a, lm, hot, alphas ? &grid : nullptr, clm);
  DS2_CHECK_LAUNCH();
  return 0;
}

int beam_stream_feed(const float* x, long stride_n, long stride_t, int N, int Tc, int C, const int* sizes, int blank, int B,
                     int cutoff_top_n, float cutoff_prob, void* state, int max_frames, int* tokens, int* offsets, long row_stride,
                     int out_ranks, int* lens, float* scores, void* ws, hipStream_t st, const LmArgs* lm, const HotArgs* hot,
                     const ClmArgs* clm) {
  DS2_REQUIRE(state && max_frames > 0 && ((long)max_frames + 1) * B <= 0x7fffffffl, DS2_ERR_ARG);
  const bool out = tokens != nullptr;
  DS2_REQUIRE(out == (offsets != nullptr) && out == (lens != nullptr) && out == (scores != nullptr), DS2_ERR_ARG);
  DS2_REQUIRE(!out || (row_stride >= 0 && out_ranks >= 1 && out_ranks <= B), DS2_ERR_ARG);
  DS2_REQUIRE(Tc > 0 ? (x && ws) : out, DS2_ERR_ARG);
  DS2_REQUIRE((((uintptr_t)ws | (uintptr_t)state) & 255) == 0, DS2_ERR_ALIGN);
  SearchArgs a;
  const int rc = beam_prune(a, x, stride_n, stride_t, N, Tc, 0, C, sizes, blank, B, cutoff_top_n, cutoff_prob, ws,
                            stream_ws_layout(N, Tc), st);
  if (rc) return rc;
  const StreamLayout SL = stream_layout(N, B, max_frames, (lm || clm ? kStreamFlagLm : 0) | (hot ? kStreamFlagHot : 0));
  char* sb = (char*)state;
  a.parent = (int*)(sb + SL.parent), a.label = (int*)(sb + SL.label), a.frame = (int*)(sb + SL.frame);
  a.tokens = tokens, a.offsets = offsets, a.lens = lens, a.scores = scores;
  launch_search_with(a, lm, hot, nullptr, clm, StreamArgs{sb, SL.state_stride, max_frames, row_stride, out_ranks});
  DS2_CHECK_LAUNCH();
  return 0;
}

}  // namespace
