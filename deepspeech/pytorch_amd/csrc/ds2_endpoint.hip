// Endpointing on the device: an endless stream of CTC posteriors is cut into utterances ("segments") at
// pauses, after long leading silence, or by length, so that the resumable beam search (ds2_beam_stream_*) starts again with an
// empty node pool and a stream can outlive max_frames.
//
// The rule is a pure function of the posteriors.  Frame t of a stream is SILENT iff x[t][blank] > blank_threshold (fp32, strict: a
// NaN is not silent).  A segment starts at frame s (0, or one past the previous endpoint).  Walking t = s, s + 1, ... with
//   trailing = the consecutive silent frames ending at t,   spoken = some frame of [s, t] was not silent,
// the segment ends at the first t where, in this order of precedence,
//   1 "silence": spoken && trailing >= min_trailing     2 "leading": !spoken && trailing >= max_leading
//   3 "length":  t - s + 1 == max_segment
// holds.  Reason 4 "final" is ds2_endpoint_close's: the caller ends the stream.
//
// k_endpoint_feed: one wave per stream, 64 frames per step (one per lane).  The ballot of the silent predicate is a 64-bit mask;
// every lane derives ITS frame's trailing / spoken from the mask with bit operations (the position of the last non-silent bit at
// or below the lane, the state's values carried in when there is none), a second ballot of "fires" and a find-first-set give the
// endpoint.  There is no serial walk over frames.  The kernel stops at the first endpoint: cut = the chunk's frames up to and
// including it, rest = the frames after it, which the caller hands to a second call (k_endpoint_gather moves them to the front of
// a second buffer) after the search of the ended streams was reset.
//
// k_endpoint_commit keeps the finished segments' output rows on the device until the host fetches them: it copies the rows that
// the beam feed's output stage wrote for an ended stream into that stream's next free ring slot.
#include "ds2_common.h"

namespace {

constexpr int kEpWords = 8;     // per-stream state: seg_start, trailing, spoken, consumed, segments, 3 reserved (int32)
constexpr int kEvWords = 4;     // an event: reason, start, end, index; events are [4][N], so the reason row is a reset mask

struct EpRule {
  float threshold;
  int min_trailing, max_leading, max_segment;
};

__global__ void __launch_bounds__(64) k_endpoint_feed(const float* __restrict__ x, long stride_n, long stride_t, int N, int Tc,
                                                      const int* __restrict__ sizes, int blank, EpRule R, int* __restrict__ state,
                                                      int* __restrict__ cut, int* __restrict__ rest, int* __restrict__ events) {
  const int n = blockIdx.x, lane = threadIdx.x;
  int size = sizes ? sizes[n] : Tc;
  size = size < 0 ? 0 : (size > Tc ? Tc : size);
  int* s = state + (long)n * kEpWords;
  if (size == 0) {                                     // the state is left bitwise as it is
    if (lane == 0) {
      cut[n] = 0;
      rest[n] = 0;
      events[n] = 0;
      events[N + n] = events[2 * N + n] = events[3 * N + n] = 0;
    }
    return;
  }
  const int seg_start = s[0], consumed = s[3], segments = s[4];
  int trailing = s[1], spoken = s[2];
  int pos = consumed - seg_start;                      // frames of the open segment before this step
  const float* xn = x + (long)n * stride_n + blank;
  for (int t0 = 0; t0 < size; t0 += 64) {
    const int t = t0 + lane;
    const bool valid = t < size;
    const bool silent = valid && xn[(long)t * stride_t] > R.threshold;   // frames at and beyond size are not read
    const unsigned long long m = __ballot(silent);
    // the last non-silent frame of this step at or below the lane: q; none -> the run reaches back into the state
    const unsigned long long upto = lane == 63 ? ~0ull : ((2ull << lane) - 1ull);
    const unsigned long long nz = ~m & upto;
    const int run = nz ? lane - (63 - __clzll((long long)nz)) : lane + 1 + trailing;
    const bool spk = nz != 0ull || spoken != 0;
    const int len = pos + lane + 1;
    int reason = 0;
    if (valid) reason = spk && run >= R.min_trailing ? 1 : (!spk && run >= R.max_leading ? 2 : (len == R.max_segment ? 3 : 0));
    const unsigned long long fire = __ballot(reason != 0);
    if (fire) {
      const int f = __ffsll((long long)fire) - 1;
      const int why = __shfl(reason, f, 64);
      if (lane == 0) {
        const int end = seg_start + pos + f;
        cut[n] = t0 + f + 1;
        rest[n] = size - (t0 + f + 1);
        events[n] = why;
        events[N + n] = seg_start;
        events[2 * N + n] = end;
        events[3 * N + n] = segments;
        s[0] = end + 1;
        s[1] = 0;
        s[2] = 0;
        s[3] = consumed + t0 + f + 1;
        s[4] = segments + 1;
      }
      return;
    }
    const int left = size - t0;
    const int last = left < 64 ? left - 1 : 63;
    trailing = __shfl(run, last, 64);
    spoken = __shfl((int)spk, last, 64);
    pos += last + 1;
  }
  if (lane == 0) {
    cut[n] = size;
    rest[n] = 0;
    events[n] = 0;
    events[N + n] = events[2 * N + n] = events[3 * N + n] = 0;
    s[1] = trailing;
    s[2] = spoken;
    s[3] = consumed + size;
  }
}

__global__ void k_endpoint_reset(int* __restrict__ state, int N, const int* __restrict__ mask) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n < N && (!mask || mask[n])) {
    int4* s = (int4*)(state + (long)n * kEpWords);
    s[0] = make_int4(0, 0, 0, 0);
    s[1] = make_int4(0, 0, 0, 0);
  }
}

// the masked streams' open segment ends here with reason 4; it may be empty (end = start - 1)
__global__ void k_endpoint_close(int* __restrict__ state, int N, const int* __restrict__ mask, int* __restrict__ events) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  int* s = state + (long)n * kEpWords;
  const bool on = !mask || mask[n];
  events[n] = on ? 4 : 0;
  events[N + n] = on ? s[0] : 0;
  events[2 * N + n] = on ? s[3] - 1 : 0;
  events[3 * N + n] = on ? s[4] : 0;
  if (on) {
    s[0] = s[3];
    s[1] = 0;
    s[2] = 0;
    s[4] += 1;
  }
}

// y[n][i] = x[n][cut[n] + i] for i < rest[n]: the frames after the endpoint, at the front of a second chunk
__global__ void __launch_bounds__(256) k_endpoint_gather(const float* __restrict__ x, long stride_n, long stride_t, int Tc, int C,
                                                         const int* __restrict__ cut, const int* __restrict__ rest,
                                                         float* __restrict__ y) {
  const int n = blockIdx.x;
  int c0 = cut[n], r = rest[n];
  c0 = c0 < 0 ? 0 : (c0 > Tc ? Tc : c0);
  r = r < 0 ? 0 : (r > Tc - c0 ? Tc - c0 : r);
  const float* xn = x + (long)n * stride_n + (long)c0 * stride_t;
  float* yn = y + (long)n * Tc * C;
  const long total = (long)r * C;
  for (long i = threadIdx.x; i < total; i += 256) {
    const long t = i / C;
    const int c = (int)(i - t * C);
    yn[i] = xn[t * stride_t + c];
  }
}

// ring: per stream `slots` slots of slot_words = 4 + 3 * ranks + 2 * ranks * row_stride int32 words:
// [reason, start, end, index][lens ranks][scores ranks][acoustic ranks][tokens ranks x row_stride][offsets ranks x row_stride]
__global__ void __launch_bounds__(256) k_endpoint_commit(const int* __restrict__ events, const int* __restrict__ tokens,
                                                         const int* __restrict__ offsets, long row_stride, int ranks,
                                                         const int* __restrict__ lens, const float* __restrict__ scores,
                                                         const float* __restrict__ acoustic, int N, int* __restrict__ ring,
                                                         int* __restrict__ pending, int slots) {
  const int n = blockIdx.x;
  if (events[n] == 0) return;
  const int slot = pending[n];
  __syncthreads();                                     // every thread has read the count before thread 0 raises it
  if (slot >= slots) return;                           // full: the host fetches before this can happen
  const long slot_words = kEvWords + 3l * ranks + 2l * ranks * row_stride;
  int* out = ring + ((long)n * slots + slot) * slot_words;
  int* olens = out + kEvWords;
  float* osc = (float*)(olens + ranks);
  float* oac = osc + ranks;
  int* otok = (int*)(oac + ranks);
  int* ooff = otok + (long)ranks * row_stride;
  if (threadIdx.x < kEvWords) out[threadIdx.x] = events[threadIdx.x * N + n];
  for (int r = threadIdx.x; r < ranks; r += 256) {
    olens[r] = lens[(long)n * ranks + r];
    osc[r] = scores[(long)n * ranks + r];
    oac[r] = acoustic ? acoustic[(long)n * ranks + r] : scores[(long)n * ranks + r];
  }
  for (int r = 0; r < ranks; ++r) {
    int len = lens[(long)n * ranks + r];
    len = len < 0 ? 0 : (len > row_stride ? (int)row_stride : len);
    const int* tk = tokens + ((long)n * ranks + r) * row_stride;
    const int* of = offsets + ((long)n * ranks + r) * row_stride;
    for (int i = threadIdx.x; i < len; i += 256) {
      otok[r * row_stride + i] = tk[i];
      ooff[r * row_stride + i] = of[i];
    }
  }
  if (threadIdx.x == 0) pending[n] = slot + 1;
}

}  // namespace

extern "C" {

long ds2_endpoint_state_bytes(int N) { return N <= 0 ? 0 : (long)N * kEpWords * 4; }

long ds2_endpoint_ring_bytes(int N, int slots, int ranks, long row_stride) {
  if (N <= 0 || slots <= 0 || ranks <= 0 || row_stride <= 0) return 0;
  return (long)N * slots * (kEvWords + 3l * ranks + 2l * ranks * row_stride) * 4;
}

// state: ds2_endpoint_state_bytes(N) bytes, 16-byte aligned.  The streams with mask[n] != 0 (device int32 [N], null = all) start
// again: segment 0 at frame 0.  A new buffer is reset as a whole before its first feed.
int ds2_endpoint_reset(void* state, int N, const int* mask, ds2_stream_t st_) {
  DS2_REQUIRE(state && N > 0, DS2_ERR_ARG);
  DS2_REQUIRE(((uintptr_t)state & 15) == 0, DS2_ERR_ALIGN);
  hipLaunchKernelGGL(k_endpoint_reset, dim3((unsigned)((N + 63) / 64)), dim3(64), 0, (hipStream_t)st_, (int*)state, N, mask);
  DS2_CHECK_LAUNCH();
  return 0;
}

// x: the chunk (N, Tc, C) with ds2_beam_stream_feed's strides; sizes [N] (device int32, null = Tc) the frames of it that each
// stream takes; frames at and beyond sizes[n] are never read.  Per stream the state advances over the frames up to and including
// the first endpoint, or over all sizes[n].  cut / rest [N] and events [4][N] (rows reason, start, end, index; all 0 without an
// endpoint) are device int32.  sizes[n] == 0 leaves the state of stream n as it is.
int ds2_endpoint_feed(const float* x, long stride_n, long stride_t, int N, int Tc, int C, const int* sizes, int blank,
                      float blank_threshold, int min_trailing, int max_leading, int max_segment, void* state, int* cut, int* rest,
                      int* events, ds2_stream_t st_) {
  DS2_REQUIRE(N > 0 && Tc > 0 && C > 0 && blank >= 0 && blank < C, DS2_ERR_ARG);
  DS2_REQUIRE(blank_threshold > 0.f && blank_threshold < 1.f, DS2_ERR_ARG);
  DS2_REQUIRE(min_trailing >= 1 && max_leading >= 1 && max_segment >= 1, DS2_ERR_ARG);
  DS2_REQUIRE(x && state && cut && rest && events, DS2_ERR_ARG);
  DS2_REQUIRE(((uintptr_t)state & 15) == 0, DS2_ERR_ALIGN);
  const EpRule R = {blank_threshold, min_trailing, max_leading, max_segment};
  hipLaunchKernelGGL(k_endpoint_feed, dim3(N), dim3(64), 0, (hipStream_t)st_, x, stride_n, stride_t, N, Tc, sizes, blank, R,
                     (int*)state, cut, rest, events);
  DS2_CHECK_LAUNCH();
  return 0;
}

// The open segment of the streams with mask[n] != 0 (null = all) ends with reason 4 ("final") at the last frame consumed; it may
// hold no frame.  events [4][N] as ds2_endpoint_feed writes them (0 for the other streams).
int ds2_endpoint_close(void* state, int N, const int* mask, int* events, ds2_stream_t st_) {
  DS2_REQUIRE(state && events && N > 0, DS2_ERR_ARG);
  DS2_REQUIRE(((uintptr_t)state & 15) == 0, DS2_ERR_ALIGN);
  hipLaunchKernelGGL(k_endpoint_close, dim3((unsigned)((N + 63) / 64)), dim3(64), 0, (hipStream_t)st_, (int*)state, N, mask, events);
  DS2_CHECK_LAUNCH();
  return 0;
}

// y (N, Tc, C) contiguous: y[n][i] = x[n][cut[n] + i] for i < rest[n]; the other frames of y are left as they are and frames of x
// at and beyond cut[n] + rest[n] are never read.
int ds2_endpoint_gather(const float* x, long stride_n, long stride_t, int N, int Tc, int C, const int* cut, const int* rest, float* y,
                        ds2_stream_t st_) {
  DS2_REQUIRE(N > 0 && Tc > 0 && C > 0, DS2_ERR_ARG);
  DS2_REQUIRE(x && cut && rest && y, DS2_ERR_ARG);
  hipLaunchKernelGGL(k_endpoint_gather, dim3(N), dim3(256), 0, (hipStream_t)st_, x, stride_n, stride_t, Tc, C, cut, rest, y);
  DS2_CHECK_LAUNCH();
  return 0;
}

// For every stream with events[0][n] != 0: the event and the rows (n, r), r < ranks, that a beam feed's output stage wrote
// (tokens / offsets row_stride ints apart, lens / scores / acoustic [N][ranks]; acoustic null = scores) go to slot pending[n] of the
// stream's ring, and pending[n] grows by one.  ring: ds2_endpoint_ring_bytes(N, slots, ranks, row_stride) bytes; pending [N] device
// int32, zeroed by the caller when it has fetched the ring.  A stream whose ring is full is skipped.
int ds2_endpoint_commit(const int* events, const int* tokens, const int* offsets, long row_stride, int ranks, const int* lens,
                        const float* scores, const float* acoustic, int N, void* ring, int* pending, int slots, ds2_stream_t st_) {
  DS2_REQUIRE(N > 0 && slots > 0 && ranks > 0 && row_stride > 0, DS2_ERR_ARG);
  DS2_REQUIRE(events && tokens && offsets && lens && scores && ring && pending, DS2_ERR_ARG);
  hipLaunchKernelGGL(k_endpoint_commit, dim3(N), dim3(256), 0, (hipStream_t)st_, events, tokens, offsets, row_stride, ranks, lens,
                     scores, acoustic, N, (int*)ring, pending, slots);
  DS2_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
