// Minimum word error rate training over an n-best list (Prabhavalkar et al. 2018): the weights that turn the per-row CTC
// gradients of ds2_ctc_multi_backward into the gradient of the expected error count.
//
// Rows are rank-major, p = k * N + n: ranks 0 .. K-1 are the clip's hypotheses, rank K (with has_ref) its reference.  Per clip, with
// A = the ranks k < K whose nll is finite and whose error count is >= 0, and s_k = -nll_k:
//   phat_k = exp(s_k - max_A s) / sum_A exp(s_j - max_A s)          the likelihoods renormalised over the list
//   risk   = ebar = sum_A phat_k err_k                              (0 when A is empty)
//   w_k    = -phat_k (err_k - ebar) = d risk / d nll_k              (0 outside A)
// and the reference row takes ce_weight (0 when its nll is infinite: zero_infinity, as the plain criterion has it) and never joins
// the softmax.  loss = sum_n risk[n] + ce_weight sum_n nll_ref[n].
//
// The work is a few dozen flops per clip, so the kernel is one workgroup and the point is a fixed order: a thread owns a clip and
// walks its ranks in index order in fp64, every output is rounded to fp32 once, and thread 0 adds the clips' fp64 terms in index
// order, a block of MWER_THREADS clips at a time.
#include <math.h>

#include "ds2_common.h"

namespace {

constexpr int MWER_THREADS = 256;

__global__ void __launch_bounds__(MWER_THREADS) k_mwer_weights(const float* __restrict__ nll, const int* __restrict__ err, int N, int K,
                                                               int has_ref, float ce_weight, float* __restrict__ weights,
                                                               float* __restrict__ risk, float* __restrict__ nll_ref,
                                                               float* __restrict__ loss) {
  __shared__ double part[2][MWER_THREADS];             // {risk, nll_ref} of the clips of the current block
  const int tid = threadIdx.x;
  double sum_risk = 0.0, sum_ref = 0.0;                // thread 0 only
  for (int n0 = 0; n0 < N; n0 += MWER_THREADS) {
    const int n = n0 + tid;
    double ebar = 0.0, ref = 0.0;
    if (n < N) {
      double smax = -INFINITY;
      for (int k = 0; k < K; ++k) {
        const float v = nll[(long)k * N + n];
        if (isfinite(v) && err[(long)k * N + n] >= 0) smax = fmax(smax, -(double)v);
      }
      double z = 0.0;
      for (int k = 0; k < K; ++k) {
        const float v = nll[(long)k * N + n];
        if (isfinite(v) && err[(long)k * N + n] >= 0) z += exp(-(double)v - smax);
      }
      for (int k = 0; k < K; ++k) {
        const float v = nll[(long)k * N + n];
        const int e = err[(long)k * N + n];
        if (isfinite(v) && e >= 0) ebar += exp(-(double)v - smax) / z * (double)e;
      }
      for (int k = 0; k < K; ++k) {
        const float v = nll[(long)k * N + n];
        const int e = err[(long)k * N + n];
        double w = 0.0;
        if (isfinite(v) && e >= 0) w = -(exp(-(double)v - smax) / z) * ((double)e - ebar);
        weights[(long)k * N + n] = (float)w;
      }
      if (has_ref) {
        const float v = nll[(long)K * N + n];
        weights[(long)K * N + n] = isfinite(v) ? ce_weight : 0.f;
        ref = isfinite(v) ? (double)v : 0.0;
      }
      risk[n] = (float)ebar;
      nll_ref[n] = (float)ref;
    }
    part[0][tid] = ebar;
    part[1][tid] = ref;
    __syncthreads();
    if (tid == 0) {
      const int cnt = N - n0 < MWER_THREADS ? N - n0 : MWER_THREADS;
      for (int i = 0; i < cnt; ++i) {
        sum_risk += part[0][i];
        sum_ref += part[1][i];
      }
    }
    __syncthreads();
  }
  if (tid == 0) *loss = (float)(sum_risk + (double)ce_weight * sum_ref);
}

}  // namespace

extern "C" {

int ds2_mwer_weights(const float* nll, const int* err, int N, int K, int has_ref, float ce_weight, float* weights, float* risk,
                     float* nll_ref, float* loss, ds2_stream_t st_) {
  DS2_REQUIRE(N > 0 && K >= 0 && (K > 0 || has_ref) && ce_weight >= 0.f && ce_weight <= 3.4028234e38f, DS2_ERR_ARG);
  DS2_REQUIRE(nll && weights && risk && nll_ref && loss && (err || K == 0), DS2_ERR_ARG);
  hipLaunchKernelGGL(k_mwer_weights, dim3(1), dim3(MWER_THREADS), 0, (hipStream_t)st_, nll, err, N, K, has_ref ? 1 : 0, ce_weight,
                     weights, risk, nll_ref, loss);
  DS2_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
