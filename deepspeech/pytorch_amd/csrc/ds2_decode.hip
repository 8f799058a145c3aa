// Greedy (arg-max) CTC decoding on the device: what validation_step does through GreedyDecoder.decode (reference
// decoder.py:164-181 over process_string :146-162, called from model.py:256): per frame the arg-max class, then per sample the
// collapse of repeats and the removal of blanks.  The reference moves the full (N, T', C) probability tensor to the host and
// walks it with one .item() per frame; here only the surviving labels and their frame offsets travel.
//
// One wave per sample; frames in chunks of 64 (one per lane): arg-max over the C classes of the lane's frame (first
// maximum wins, like torch.max), keep = label != blank && (t == 0 || label != label of frame t-1) && t < size, compaction by
// ballot + popcount prefix.  HBM-bound: reads N*T'*C floats once (the rows are 116-256 bytes, each lane streams its own row).
//
// k_greedy_stream (ds2_greedy_stream_feed) is the same rule on one chunk of a stream: the carry (arg-max of the stream's last
// frame, frames consumed) lives in device memory between the calls, the offsets count from the start of the stream, and only the
// labels that the chunk adds are written.  Greedy output is append-only, so the chunks' outputs concatenate to the one-shot output.
#include "ds2_common.h"

namespace {

__global__ void __launch_bounds__(64) k_greedy_decode(const float* __restrict__ x, long stride_n, long stride_t, int T, int C,
                                                      const int* __restrict__ sizes, int blank, int* __restrict__ tokens,
                                                      int* __restrict__ offsets, int* __restrict__ counts) {
  const int n = blockIdx.x, lane = threadIdx.x;
  int size = sizes ? sizes[n] : T;
  size = size < 0 ? 0 : (size > T ? T : size);
  const float* xn = x + (long)n * stride_n;
  int* tok = tokens + (long)n * T;
  int* off = offsets + (long)n * T;
  int count = 0;
  int carry = -1;                                      // arg-max of the frame before this chunk (none before frame 0)
  for (int t0 = 0; t0 < size; t0 += 64) {
    const int t = t0 + lane;
    int best = -1;
    if (t < size) {
      const float* row = xn + (long)t * stride_t;
      float bv = row[0];
      best = 0;
      for (int c = 1; c < C; ++c) {
        const float v = row[c];
        if (v > bv) {
          bv = v;
          best = c;
        }
      }
    }
    int prev = __shfl_up(best, 1, 64);
    if (lane == 0) prev = carry;
    const bool keep = t < size && best != blank && (t == 0 || best != prev);
    const unsigned long long m = __ballot(keep);
    if (keep) {
      const int pos = count + __popcll(m & ((1ull << lane) - 1ull));
      tok[pos] = best;
      off[pos] = t;
    }
    count += __popcll(m);
    carry = __shfl(best, 63, 64);
  }
  if (lane == 0) counts[n] = count;
}

// carry: [N][2] = (arg-max of the stream's last frame, frames consumed); a stream with no frames consumed has no previous label
__global__ void __launch_bounds__(64) k_greedy_stream(const float* __restrict__ x, long stride_n, long stride_t, int T, int C,
                                                      const int* __restrict__ sizes, int blank, int* __restrict__ carry_,
                                                      int* __restrict__ tokens, int* __restrict__ offsets,
                                                      int* __restrict__ counts) {
  const int n = blockIdx.x, lane = threadIdx.x;
  int size = sizes ? sizes[n] : T;
  size = size < 0 ? 0 : (size > T ? T : size);
  const float* xn = x + (long)n * stride_n;
  int* tok = tokens + (long)n * T;
  int* off = offsets + (long)n * T;
  int count = 0;
  int carry = carry_[2 * n];
  const int done = carry_[2 * n + 1];                  // frames before this chunk
  for (int t0 = 0; t0 < size; t0 += 64) {
    const int t = t0 + lane;
    int best = -1;
    if (t < size) {
      const float* row = xn + (long)t * stride_t;
      float bv = row[0];
      best = 0;
      for (int c = 1; c < C; ++c) {
        const float v = row[c];
        if (v > bv) {
          bv = v;
          best = c;
        }
      }
    }
    int prev = __shfl_up(best, 1, 64);
    if (lane == 0) prev = carry;
    const bool keep = t < size && best != blank && (done + t == 0 || best != prev);
    const unsigned long long m = __ballot(keep);
    if (keep) {
      const int pos = count + __popcll(m & ((1ull << lane) - 1ull));
      tok[pos] = best;
      off[pos] = done + t;
    }
    count += __popcll(m);
    const int left = size - t0;                        // the last frame of the chunk may sit below lane 63
    carry = __shfl(best, left < 64 ? left - 1 : 63, 64);
  }
  if (lane == 0) {
    counts[n] = count;
    if (size > 0) {
      carry_[2 * n] = carry;
      carry_[2 * n + 1] = done + size;
    }
  }
}

}  // namespace

extern "C" {

// x: scores (probabilities or logits) of sample n, frame t, class c at x[n*stride_n + t*stride_t + c] (f32; any (N,T',C)
// view whose class dimension is contiguous).  sizes: [N] valid frames per sample (device int32, may be null = T).
// Outputs (device int32): tokens [N][T], offsets [N][T] (first `counts[n]` entries of row n are valid), counts [N].
int ds2_greedy_decode(const float* x, long stride_n, long stride_t, int N, int T, int C, const int* sizes, int blank,
                      int* tokens, int* offsets, int* counts, ds2_stream_t st_) {
  hipStream_t st = (hipStream_t)st_;
  DS2_REQUIRE(N > 0 && T > 0 && C > 0 && blank >= 0 && blank < C, DS2_ERR_ARG);
  DS2_REQUIRE(x && tokens && offsets && counts, DS2_ERR_ARG);
  hipLaunchKernelGGL(k_greedy_decode, dim3(N), dim3(64), 0, st, x, stride_n, stride_t, T, C, sizes, blank, tokens, offsets, counts);
  DS2_CHECK_LAUNCH();
  return 0;
}

// ds2_greedy_decode on one chunk (N, Tc, C) of N streams.  carry: [N][2] device int32 (arg-max of the stream's last frame, frames
// consumed), all zero for a fresh stream and updated by the call; sizes[n] == 0 leaves stream n as it is.  tokens / offsets [N][Tc]:
// the counts[n] labels that this chunk adds to stream n and their frames counted from the start of the stream.  Tc >= 1 (there is
// no output stage to run alone, unlike ds2_beam_stream_feed); the int32 frame counter is not bounded here.
int ds2_greedy_stream_feed(const float* x, long stride_n, long stride_t, int N, int Tc, int C, const int* sizes, int blank,
                           int* carry, int* tokens, int* offsets, int* counts, ds2_stream_t st_) {
  hipStream_t st = (hipStream_t)st_;
  DS2_REQUIRE(N > 0 && Tc > 0 && C > 0 && blank >= 0 && blank < C, DS2_ERR_ARG);
  DS2_REQUIRE(x && carry && tokens && offsets && counts, DS2_ERR_ARG);
  hipLaunchKernelGGL(k_greedy_stream, dim3(N), dim3(64), 0, st, x, stride_n, stride_t, Tc, C, sizes, blank, carry, tokens, offsets,
                     counts);
  DS2_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
