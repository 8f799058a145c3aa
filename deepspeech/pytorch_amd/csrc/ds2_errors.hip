// Character and word error counts on the device: the edit distances behind decoder.CharErrorRate / decoder.WordErrorRate
// (reference validation.py:66-132), for a grid of hypotheses against a batch of references, so that a language-model weight
// search (lm_search.py) never brings a transcript to the host.
//
// One launch, one wave per pair p = (hypothesis p, reference p % R):
//   1  both label strings are compacted into LDS twice: the labels that are not the space (the metric's replace(' ', '')), and one
//      61-bit hash per word (a maximal run of non-space labels, which is str.split(); the hash is the beam search's string hash,
//      ds2_strhash.h, started at the empty string for every word).  Positions come from wave ballots; the lane that holds a word's
//      first label hashes the word.
//   2  Levenshtein distance of the two compacted strings, then of the two hash strings.  The reference string is cut into strips
//      of 64 columns, one column per lane; lane l works on row s - l in step s (a skewed wavefront), so that the cell to its left
//      and the one diagonally above are the last two values of lane l - 1, fetched with two wave shifts.  Lane 0 takes them from
//      the previous strip's last column, which lane 63 leaves in LDS (edge[]) 63 steps after lane 0 read that row.
// Every loop is bounded by a length, and every length is clamped to ERR_MAXLEN before it is used.
#include "ds2_common.h"
#include "ds2_strhash.h"

#define ERR_MAXLEN 4096
#define ERR_MAXWORDS (ERR_MAXLEN / 2)   // a word takes a label and, all but the last, a space

namespace {

// seq[0 .. len) -> chars[0 .. nchars) (labels other than the space) and words[0 .. nwords) (one hash per word)
__device__ __forceinline__ void compact(const int* __restrict__ seq, int len, int space, int* chars, uint64_t* words, int lane,
                                        int& nchars, int& nwords) {
  int nc = 0, nw = 0;
  const unsigned long long below = (1ull << lane) - 1;
  for (int base = 0; base < len; base += 64) {
    const int p = base + lane;
    const bool in = p < len;
    const int x = in ? seq[p] : space;
    const bool ch = in && x != space;
    const bool start = ch && (p == 0 || seq[p - 1] == space);
    const unsigned long long mc = __ballot(ch), ms = __ballot(start);
    if (ch) chars[nc + __popcll(mc & below)] = x;
    if (start) {
      uint64_t h = kHashEmpty;
      for (int q = p; q < len; ++q) {
        const int y = seq[q];
        if (y == space) break;
        h = hash_ext(h, y);
      }
      words[nw + __popcll(ms & below)] = h;
    }
    nc += __popcll(mc);
    nw += __popcll(ms);
  }
  nchars = nc;
  nwords = nw;
}

// D[i][j] = distance of a[0 .. i) and b[0 .. j); returns D[m][n].  edge[i] holds D[i][j0] of the strip at work, i = 1 .. m.
template <class E>
__device__ __forceinline__ int edit_distance(const E* a, int m, const E* b, int n, int* edge, int lane) {
  for (int i = lane; i <= m; i += 64) edge[i] = i;
  __syncthreads();
  int res = m;   // n == 0
  for (int j0 = 0; j0 < n; j0 += 64) {
    const int width = n - j0 < 64 ? n - j0 : 64;
    const int j = j0 + lane + 1;
    const bool col = lane < width;
    const E bj = col ? b[j - 1] : E(0);
    int v1 = j, v2 = j;    // D[i][j], D[i - 1][j] of the row this lane finished last (row 0: D[0][j] = j)
    int above = j0;        // lane 0: D[i - 1][j0]
    for (int s = 1; s < m + width; ++s) {
      const int i = s - lane;
      int left = __shfl_up(v1, 1, 64), diag = __shfl_up(v2, 1, 64);
      if (lane == 0) {
        left = i <= m ? edge[i] : 0;
        diag = above;
      }
      if (col && i >= 1 && i <= m) {
        const int up = v1 + 1, lf = left + 1, dg = diag + (a[i - 1] != bj);
        const int v = up < lf ? (up < dg ? up : dg) : (lf < dg ? lf : dg);
        v2 = v1;
        v1 = v;
        above = left;
        if (lane == 63) edge[i] = v;
      }
    }
    __syncthreads();
    res = __shfl(v1, width - 1, 64);
  }
  return res;
}

__global__ void __launch_bounds__(64) k_error_counts(const int* __restrict__ hyp, long hyp_stride, const int* __restrict__ hyp_lens,
                                                     const int* __restrict__ ref, const int* __restrict__ ref_offsets, int R,
                                                     int space, int* __restrict__ char_err, int* __restrict__ word_err,
                                                     int* __restrict__ ref_chars, int* __restrict__ ref_words) {
  __shared__ int hc[ERR_MAXLEN], rc[ERR_MAXLEN], edge[ERR_MAXLEN + 1];
  __shared__ uint64_t hw[ERR_MAXWORDS], rw[ERR_MAXWORDS];
  const int p = blockIdx.x, lane = threadIdx.x, r = p % R;
  const int hl = hyp_lens[p];
  const long r0 = ref_offsets[r], rl = (long)ref_offsets[r + 1] - r0;
  if (hl < 0 || hl > ERR_MAXLEN || (long)hl > hyp_stride || r0 < 0 || rl < 0 || rl > ERR_MAXLEN) {
    // a length the host could not see and this kernel does not take: the pair is marked, nothing of it is read
    if (lane == 0) {
      char_err[p] = -1;
      word_err[p] = -1;
      if (p < R) {
        ref_chars[p] = -1;
        ref_words[p] = -1;
      }
    }
    return;
  }
  int m, mw, n, nw;
  compact(hyp + (long)p * hyp_stride, hl, space, hc, hw, lane, m, mw);
  compact(ref + r0, (int)rl, space, rc, rw, lane, n, nw);
  __syncthreads();
  const int ce = edit_distance(hc, m, rc, n, edge, lane);
  __syncthreads();
  const int we = edit_distance(hw, mw, rw, nw, edge, lane);
  if (lane == 0) {
    char_err[p] = ce;
    word_err[p] = we;
    if (p < R) {
      ref_chars[p] = n;
      ref_words[p] = nw;
    }
  }
}

}  // namespace

extern "C" {

// hyp: P rows of labels, row p at hyp + p * hyp_stride with hyp_lens[p] labels; ref: the references' labels back to back,
// reference r at ref[ref_offsets[r] .. ref_offsets[r + 1]).  Pair p is (hypothesis p, reference p % R).  All pointers are device
// memory; char_err / word_err [P], ref_chars / ref_words [R].  Labels are non-negative.
int ds2_error_counts(const int* hyp, long hyp_stride, const int* hyp_lens, int P, const int* ref, const int* ref_offsets, int R,
                     int space, int* char_err, int* word_err, int* ref_chars, int* ref_words, ds2_stream_t st_) {
  DS2_REQUIRE(P >= 1 && R >= 1 && R <= P && hyp_stride >= 0, DS2_ERR_ARG);
  DS2_REQUIRE(hyp && hyp_lens && ref && ref_offsets && char_err && word_err && ref_chars && ref_words, DS2_ERR_ARG);
  hipLaunchKernelGGL(k_error_counts, dim3((unsigned)P), dim3(64), 0, (hipStream_t)st_, hyp, hyp_stride, hyp_lens, ref, ref_offsets,
                     R, space, char_err, word_err, ref_chars, ref_words);
  DS2_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
