// The output layer (model.py:195-201: Linear(H, C, bias=False) after the BatchNorm) for at most 64 padded classes.  A product with 32
// or 64 output columns is HBM-bound on the [R][H] activation matrix: the generic 128x128 kernels spend a tile on it and the backward
// needed two operand transposes and a K-sliced product.  Here every pass reads (or writes) the activations once, in 16-byte pieces:
//   k_fc_fwd   logits[R][Cp] f32 = Xh[R][H] * Wp[Cp][H]^T, Wp resident in LDS in MFMA fragment order
//   k_fc_dx    dXh[R][H] = bf16(dlogits) * Wp from dlogits as stored (no cast pass, no transposed weight)
//   k_fc_dw    the fp32 partial sums of dW = bf16(dlogits)^T * Xh per row block from both operands as stored (no transposes);
//              k_fc_sum_partials adds the partials in index order (no atomics: the same bits in every run)
// All products run on v_mfma_f32_32x32x16_bf16 in the k-steps, order and operand slots of the generic kernels they replace on this
// layer (ds2_gemm.hip), so the step computes the same bits as with those.
#include "ds2_common.h"

namespace {

typedef short fc_s16x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) fc_s16x4* fc_lds_s16x4_ptr;

__device__ __forceinline__ uint4 fc_ld16(const uint16_t* p) { return *reinterpret_cast<const uint4*>(p); }

// ---- forward -------------------------------------------------------------------------------------------------------------------
// A wave owns a 32-row tile; its lane (r = lane & 31, hh = lane >> 5) reads the 16-byte pieces 2 i + hh (i = 0..3) of every 128-byte
// segment q of row r -- four loads that, over the two lane halves, consume whole 128-byte lines -- and MFMA step 4 q + i contracts
// over k = 16 (4 q + i) + 8 hh + j (j = 0..7), with the weight in the first operand slot: the k-steps, their order and the operand
// slots of k_gemm_nt_bf16_glds, so the logits keep the bits the generic kernel gave them.  The LDS image of Wp is stored in fragment
// order, [step][class tile][lane][16 bytes], so a fragment read is one lane-linear ds_read_b128.  k >= H is zero on both sides
// (H % 8 == 0: a piece is whole or absent).
template <int NT>   // class tiles of 32
__global__ void __launch_bounds__(256) k_fc_fwd(const uint16_t* __restrict__ X, long ldx, const uint16_t* __restrict__ W, long ldw,
                                                float* __restrict__ out, long ldo, int R, int H) {
  extern __shared__ __attribute__((aligned(16))) unsigned char fc_smem[];
  uint4* wl = reinterpret_cast<uint4*>(fc_smem);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nwave = blockDim.x >> 6;
  const int NQ = (H + 63) >> 6, ppr = NQ * 8;        // 16-byte pieces per (zero-extended) row of Wp
  // eight loads in flight per thread (the image is 64 KiB at H = 1024: one load per trip would be a chain of L2 round trips)
  const int npiece = NT * 32 * ppr, nthr = blockDim.x;
  for (int base = tid; base < npiece; base += 8 * nthr) {
    uint4 v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int idx = min(base + u * nthr, npiece - 1), c = idx / ppr, kp = idx - c * ppr;
      const uint4 x = fc_ld16(W + (long)c * ldw + min(kp * 8, H - 8));
      v[u] = kp * 8 < H ? x : make_uint4(0, 0, 0, 0);
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int idx = base + u * nthr;
      if (idx < npiece) {
        const int c = idx / ppr, kp = idx - c * ppr;
        const int q = kp >> 3, i = (kp >> 1) & 3, hh = kp & 1;
        wl[(((q * 4 + i) * NT + (c >> 5)) << 6) + hh * 32 + (c & 31)] = v[u];
      }
    }
  }
  __syncthreads();
  const int ntile = (R + 31) >> 5, r = lane & 31, hh = lane >> 5;
  const int NQfull = H >> 6;
  for (int tile = blockIdx.x * nwave + wave; tile < ntile; tile += gridDim.x * nwave) {
    const int row = min(tile * 32 + r, R - 1);       // rows past the end repeat the last one; they are not stored
    const uint16_t* xp = X + (long)row * ldx + hh * 8;
    ds2_f32x16 acc[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[nt][e] = 0.f;
    // QB segments = 4 QB loads (32 KiB per wave at QB = 8) are issued before the first product: a wave has one tile or few, so
    // nothing else hides the latency.  The fence keeps the compiler from sinking the loads between the MFMAs again.
    constexpr int QB = 8;
    int q = 0;
    for (; q + QB <= NQfull; q += QB) {
      uint4 a[QB][4];
#pragma unroll
      for (int u = 0; u < QB; ++u)
#pragma unroll
        for (int i = 0; i < 4; ++i) a[u][i] = fc_ld16(xp + (q + u) * 64 + i * 16);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int u = 0; u < QB; ++u)
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int nt = 0; nt < NT; ++nt) Mma<bf16_t>::mma32(acc[nt], wl[((((q + u) * 4 + i) * NT + nt) << 6) + lane], a[u][i]);
    }
    for (; q < NQfull; ++q) {
      uint4 a[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) a[i] = fc_ld16(xp + q * 64 + i * 16);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) Mma<bf16_t>::mma32(acc[nt], wl[(((q * 4 + i) * NT + nt) << 6) + lane], a[i]);
    }
    if (NQfull < NQ) {                               // the last, partial 64-column segment (q == NQfull)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        uint4 a = make_uint4(0, 0, 0, 0);
        if (q * 64 + i * 16 + hh * 8 < H) a = fc_ld16(xp + q * 64 + i * 16);
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) Mma<bf16_t>::mma32(acc[nt], wl[(((q * 4 + i) * NT + nt) << 6) + lane], a);
      }
    }
    // D[class][row]: a lane holds its row's classes 8 g4 + 4 hh .. + 3 of every class tile in registers 4 g4 .. 4 g4 + 3
    if (tile * 32 + r < R) {
#pragma unroll
      for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4)
          *reinterpret_cast<float4*>(out + (long)(tile * 32 + r) * ldo + nt * 32 + 8 * g4 + 4 * hh) =
              make_float4(acc[nt][4 * g4], acc[nt][4 * g4 + 1], acc[nt][4 * g4 + 2], acc[nt][4 * g4 + 3]);
    }
  }
}

// ---- backward ------------------------------------------------------------------------------------------------------------------
// Every product keeps the k-steps (16 wide, in index order, one accumulator), the operand slots and -- for dW -- the K-slices of the
// generic path it replaces (ops.gemm_nt on bf16(dlogits) and W^T; transposes + ops.gemm_nt_kslices + ds2_sum_slices) when the
// caller passes that path's slice length as the row block (ops.fc_bwd does: one place decides the slices), so dXh and dW keep their bits.  What goes is the traffic: no cast pass, no transposes of dlogits and Xh, Xh read once, dXh written once.
//
// k_fc_dx: dXh[R][H] = bf16(dlogits) * Wp.  One wave per workgroup (p, panel): gb groups of 32 rows x 64 columns; its W^T
// fragments stay in registers.  D[row][h] has a lane's column h in its registers by rows: the tile goes through a wave-private LDS
// piece (2-byte writes) and leaves in 16-byte pieces, 8 lanes per 128-byte line (64 threads: the barriers are wave barriers).
constexpr int FCB_LDR = 144;                 // bytes per LDS row of a [32][64] bf16 piece (128 + 16: rows fall on shifted banks)
constexpr int FCB_PIECE = 32 * FCB_LDR;

template <int MT>   // class tiles of 32
__global__ void __launch_bounds__(64) k_fc_dx(const float* __restrict__ dl, long ldg, const uint16_t* __restrict__ W, long ldw,
                                               uint16_t* __restrict__ dX, long lddx, int R, int H, int gb) {
  constexpr int KS = 2 * MT;                 // 16-class k-steps
  __shared__ __attribute__((aligned(16))) unsigned char bufy[FCB_PIECE];
  const int lane = threadIdx.x, li = lane & 31, hh = lane >> 5;
  const int h0 = blockIdx.y * 64;
  const int g0 = blockIdx.x * gb, g1 = min(g0 + gb, (R + 31) >> 5);

  // Wp^T fragments (second operand slot): lane (h = li, hh) of column tile nt, k-step s holds Wp[s * 16 + 8 hh + j][h0 + nt * 32 + h]
  uint4 wf[2][KS];
#pragma unroll
  for (int nt = 0; nt < 2; ++nt)
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      const int h = h0 + nt * 32 + li, hc = min(h, H - 1);          // unconditional loads (clamped column), then a select: a load
      uint32_t e[8];                                                // behind a branch would wait for the one before it
#pragma unroll
      for (int j = 0; j < 8; ++j) e[j] = (uint32_t)W[(long)(s * 16 + 8 * hh + j) * ldw + hc];
      const uint4 f = make_uint4(e[0] | (e[1] << 16), e[2] | (e[3] << 16), e[4] | (e[5] << 16), e[6] | (e[7] << 16));
      wf[nt][s] = h < H ? f : make_uint4(0, 0, 0, 0);
    }
  const int prow = lane >> 3, pc = lane & 7;   // the 16-byte piece pc of row prow + 8 it a lane stores
  const bool pcol_ok = h0 + pc * 8 < H;
  const int pcol = pcol_ok ? h0 + pc * 8 : 0;
  for (int g = g0; g < g1; ++g) {
    // bf16(dl) in the first operand slot: lane (row = li, hh), k-step s holds dl[g * 32 + row][s * 16 + 8 hh + j]
    uint4 db[KS];
    const int row = g * 32 + li;
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      const float* p = dl + (long)min(row, R - 1) * ldg + s * 16 + 8 * hh;
      const float4 u0 = *reinterpret_cast<const float4*>(p), u1 = *reinterpret_cast<const float4*>(p + 4);
      db[s] = make_uint4(cvt_pk_bf16(u0.x, u0.y), cvt_pk_bf16(u0.z, u0.w), cvt_pk_bf16(u1.x, u1.y), cvt_pk_bf16(u1.z, u1.w));
    }
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
      ds2_f32x16 d;
#pragma unroll
      for (int e = 0; e < 16; ++e) d[e] = 0.f;
#pragma unroll
      for (int s = 0; s < KS; ++s) Mma<bf16_t>::mma32(d, db[s], wf[nt][s]);
#pragma unroll
      for (int e = 0; e < 16; ++e)
        *reinterpret_cast<uint16_t*>(bufy + mma32_row(e, lane) * FCB_LDR + (nt * 32 + li) * 2) = (uint16_t)cvt_pk_bf16(d[e], 0.f);
    }
    __syncthreads();
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const int orow = g * 32 + it * 8 + prow;
      const uint4 v = *reinterpret_cast<const uint4*>(bufy + (it * 8 + prow) * FCB_LDR + pc * 16);
      if (pcol_ok && orow < R) *reinterpret_cast<uint4*>(dX + (long)orow * lddx + pcol) = v;
    }
    __syncthreads();
  }
}

// k_fc_dw: one wave per (row block p, 32 columns): part[p][c][h] = sum over the block's rows of bf16(dl)[r][c] * Xh[r][h], 16 rows per
// MFMA in row order -- a chain as long as the block, so the only parallelism is across blocks and column tiles, and a wave hides the
// latency itself: a ring of G row groups (32 rows each: its [32][32] piece of Xh, 16-byte loads, and its dl fragments) is in flight, and
// a slot is refilled as soon as it has been consumed.  The piece goes to LDS as loaded and ds_read_b64_tr_b16 hands it back with the
// rows as the contraction index.  Rows >= R and columns >= H are zero.
template <int MT>
__global__ void __launch_bounds__(64) k_fc_dw(const float* __restrict__ dl, long ldg, const uint16_t* __restrict__ X, long ldx,
                                              float* __restrict__ part, int R, int H, int gb) {
  constexpr int G = MT == 1 ? 8 : 4;
  constexpr int XLD = 64;                    // bytes per LDS row of the [32][32] piece: the 4 rows x 64 bytes of a transposed read tile the banks
  __shared__ __attribute__((aligned(16))) unsigned char bufx[32 * XLD];
  const int lane = threadIdx.x, li = lane & 31, hh = lane >> 5;
  const int h0 = blockIdx.y * 32;
  const int g0 = blockIdx.x * gb, g1 = min(g0 + gb, (R + 31) >> 5);
  const int prow = lane >> 2, pc = lane & 3;   // 16-byte piece pc of row prow + 16 it
  const bool pcol_ok = h0 + pc * 8 < H;
  const int pcol = pcol_ok ? h0 + pc * 8 : 0;
  const int l16 = lane & 15, gq = lane >> 4;   // transposed read: see ds_read_b64_tr_b16 in ds2_gemm8.hip
  const unsigned char* tr = bufx + (8 * (gq >> 1) + (l16 >> 2)) * XLD + (16 * (gq & 1) + 4 * (l16 & 3)) * 2;

  uint4 xr[G][2];
  float dr[G][2][MT][8];
  // A wave is alone on its SIMD, so every address instruction is exposed: a whole group (all 32 rows < R) is loaded from a uniform
  // row pointer plus a per-lane 32-bit offset, without clamps; only the last, partial group of the matrix takes the clamped form.
  const unsigned dvo = (unsigned)(8 * hh) * (unsigned)ldg + li, xvo = (unsigned)prow * (unsigned)ldx + pcol;
  auto issue = [&](int u, int g) {           // loads of group g into slot u
    if (g * 32 + 32 <= R) {
      const float* db_ = dl + (long)g * 32 * ldg;
      const uint16_t* xb_ = X + (long)g * 32 * ldx;
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
          for (int j = 0; j < 8; ++j) dr[u][ks][mt][j] = (db_ + (long)(ks * 16 + j) * ldg + mt * 32)[dvo];
#pragma unroll
      for (int it = 0; it < 2; ++it) xr[u][it] = fc_ld16(xb_ + (long)it * 16 * ldx + xvo);
    } else {
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
          for (int j = 0; j < 8; ++j) dr[u][ks][mt][j] = dl[(long)min(g * 32 + ks * 16 + 8 * hh + j, R - 1) * ldg + mt * 32 + li];
#pragma unroll
      for (int it = 0; it < 2; ++it) xr[u][it] = fc_ld16(X + (long)min(g * 32 + it * 16 + prow, R - 1) * ldx + pcol);
    }
  };
  ds2_f32x16 acc[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[mt][e] = 0.f;
#pragma unroll
  for (int u = 0; u < G; ++u) issue(u, g0 + u);
  for (int gm = g0; gm < g1; gm += G) {
#pragma unroll
    for (int u = 0; u < G; ++u) {
      const int g = gm + u;
      if (g < g1) {                          // uniform over the wave
        const bool whole = g * 32 + 32 <= R;  // uniform: no row masks
        uint4 da[2][MT];                     // bf16(dl), second operand slot: lane (c = li, hh), k-step ks: rows g * 32 + 16 ks + 8 hh + j
        if (whole) {
#pragma unroll
          for (int it = 0; it < 2; ++it)
            *reinterpret_cast<uint4*>(bufx + (it * 16 + prow) * XLD + pc * 16) = pcol_ok ? xr[u][it] : make_uint4(0, 0, 0, 0);
#pragma unroll
          for (int ks = 0; ks < 2; ++ks)
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
              const float* v = dr[u][ks][mt];
              da[ks][mt] = make_uint4(cvt_pk_bf16(v[0], v[1]), cvt_pk_bf16(v[2], v[3]), cvt_pk_bf16(v[4], v[5]), cvt_pk_bf16(v[6], v[7]));
            }
        } else {
#pragma unroll
          for (int it = 0; it < 2; ++it)
            *reinterpret_cast<uint4*>(bufx + (it * 16 + prow) * XLD + pc * 16) =
                pcol_ok && g * 32 + it * 16 + prow < R ? xr[u][it] : make_uint4(0, 0, 0, 0);
#pragma unroll
          for (int ks = 0; ks < 2; ++ks)
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
              float v[8];
#pragma unroll
              for (int j = 0; j < 8; ++j) v[j] = g * 32 + ks * 16 + 8 * hh + j < R ? dr[u][ks][mt][j] : 0.f;
              da[ks][mt] = make_uint4(cvt_pk_bf16(v[0], v[1]), cvt_pk_bf16(v[2], v[3]), cvt_pk_bf16(v[4], v[5]), cvt_pk_bf16(v[6], v[7]));
            }
        }
        // refilled unconditionally: the last G groups of a row block fetch (clamped, unused) rows past it -- 16 KB per wave.  Behind
        // a `g + G < g1` test the compiler no longer knows how many loads are in flight at the next use and waits for all of them:
        // 52.8 instead of 37.6 us at cfg3 (profiles/pr_fc_tail_kernels.md)
        issue(u, g + G);
        __syncthreads();
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
          const fc_s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((fc_lds_s16x4_ptr)(tr + ks * 16 * XLD));
          const fc_s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((fc_lds_s16x4_ptr)(tr + (ks * 16 + 4) * XLD));
          const uint2 l2 = __builtin_bit_cast(uint2, lo), h2 = __builtin_bit_cast(uint2, hi);
          const uint4 xb = make_uint4(l2.x, l2.y, h2.x, h2.y);   // Xh, first operand slot: lane (h = li, hh), rows 16 ks + 8 hh + j
#pragma unroll
          for (int mt = 0; mt < MT; ++mt) Mma<bf16_t>::mma32(acc[mt], xb, da[ks][mt]);
        }
        __syncthreads();
      }
    }
  }
  // D[h][c]: lane (c = li, hh) holds columns h0 + 8 g4 + 4 hh .. + 3 in registers 4 g4 .. 4 g4 + 3
  const int Cp = MT * 32;
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int h = h0 + mma32_row(e, lane);
      if (h < H) part[((long)blockIdx.x * Cp + mt * 32 + li) * H + h] = acc[mt][e];
    }
}

// dW[i] = sum over the row blocks p = 0 .. P-1 of part[p][i], added in that order; one thread per element, up to 32 loads in flight
template <int B>
__device__ __forceinline__ void fc_sum_batch(const float* __restrict__ src, long n, int& p, int P, float& s) {
  for (; p + B <= P; p += B) {
    float x[B];
#pragma unroll
    for (int k = 0; k < B; ++k) x[k] = src[(long)(p + k) * n];
#pragma unroll
    for (int k = 0; k < B; ++k) s += x[k];
  }
}
__global__ void __launch_bounds__(256) k_fc_sum_partials(const float* __restrict__ part, float* __restrict__ dW, int n, int P) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float s = 0.f;
  int p = 0;
  fc_sum_batch<32>(part + i, n, p, P, s);
  fc_sum_batch<8>(part + i, n, p, P, s);
  fc_sum_batch<1>(part + i, n, p, P, s);
  dW[i] = s;
}

constexpr long FC_MAX_LDS = 128 * 1024;      // the forward's resident image of Wp
inline long fc_fwd_lds(int H, int Cp) { return (long)((H + 63) / 64 * 64) * Cp * 2; }
inline bool fc_shape_ok(int H, int Cp) { return (Cp == 32 || Cp == 64) && H > 0 && H % 8 == 0 && fc_fwd_lds(H, Cp) <= FC_MAX_LDS; }
// 32-row groups per workgroup of k_fc_dx: about eight waves per compute unit over all column panels
inline int fc_dx_gb(long R, int H) {
  const int groups = ds2_cdiv(R, 32), panels = ds2_cdiv(H, 64);
  const int want = 8 * ds2_cu_count() / panels;
  return ds2_cdiv(groups, want < 1 ? 1 : want);
}

}  // namespace

extern "C" {

int ds2_fc_supported(int H, int Cp) { return fc_shape_ok(H, Cp) ? 1 : 0; }

int ds2_fc_fwd(const void* Xh, long ldx, const void* Wp, long ldw, float* logits, long ldl, long R, int H, int Cp, ds2_stream_t st_) {
  hipStream_t st = (hipStream_t)st_;
  DS2_REQUIRE(Xh && Wp && logits && R > 0 && R < (1L << 31) - 64, DS2_ERR_ARG);
  DS2_REQUIRE(fc_shape_ok(H, Cp) && ldx >= H && ldw >= H && ldl >= Cp, DS2_ERR_ARG);
  DS2_REQUIRE(ldx % 8 == 0 && ldw % 8 == 0 && ldl % 4 == 0 && ((((uintptr_t)Xh) | ((uintptr_t)Wp) | ((uintptr_t)logits)) & 15) == 0, DS2_ERR_ALIGN);
  const int shm = (int)fc_fwd_lds(H, Cp);
  const int ntile = ds2_cdiv(R, 32), cus = ds2_cu_count();
  // up to four waves per workgroup, fewer when that leaves compute units without a tile
  int waves = ds2_cdiv(ntile, cus);
  waves = waves < 1 ? 1 : waves > 4 ? 4 : waves;
  int grid = ds2_cdiv(ntile, waves);
  if (grid > 2 * cus) grid = 2 * cus;
  static bool attr1[DS2_MAX_DEVICES], attr2[DS2_MAX_DEVICES];
  if (Cp == 32) {
    if (ds2_first_use_on_device(attr1)) (void)hipFuncSetAttribute((const void*)k_fc_fwd<1>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)FC_MAX_LDS);
    hipLaunchKernelGGL(k_fc_fwd<1>, dim3(grid), dim3(64 * waves), shm, st, (const uint16_t*)Xh, ldx, (const uint16_t*)Wp, ldw, logits, ldl, (int)R, H);
  } else {
    if (ds2_first_use_on_device(attr2)) (void)hipFuncSetAttribute((const void*)k_fc_fwd<2>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)FC_MAX_LDS);
    hipLaunchKernelGGL(k_fc_fwd<2>, dim3(grid), dim3(64 * waves), shm, st, (const uint16_t*)Xh, ldx, (const uint16_t*)Wp, ldw, logits, ldl, (int)R, H);
  }
  DS2_CHECK_LAUNCH();
  return 0;
}

long ds2_fc_bwd_partials(long R, long block_rows) {
  if (R <= 0 || block_rows <= 0) return 0;
  return (R + block_rows - 1) / block_rows;
}

int ds2_fc_bwd(const float* dlogits, long ldg, const void* Xh, long ldx, const void* Wp, long ldw, void* dXh, long lddx, float* dW,
               float* ws, long R, int H, int Cp, long block_rows, ds2_stream_t st_) {
  hipStream_t st = (hipStream_t)st_;
  DS2_REQUIRE(dlogits && Xh && Wp && dXh && dW && ws && R > 0 && R < (1L << 31) - 64 * 64, DS2_ERR_ARG);
  DS2_REQUIRE(fc_shape_ok(H, Cp) && ldg >= Cp && ldx >= H && ldw >= H && lddx >= H && block_rows > 0 && block_rows % 32 == 0, DS2_ERR_ARG);
  DS2_REQUIRE(ldg % 4 == 0 && ldx % 8 == 0 && lddx % 8 == 0 &&
                  ((((uintptr_t)dlogits) | ((uintptr_t)Xh) | ((uintptr_t)dXh) | ((uintptr_t)ws) | ((uintptr_t)dW)) & 15) == 0 &&
                  (((uintptr_t)Wp) & 1) == 0, DS2_ERR_ALIGN);
  const int gx = fc_dx_gb(R, H), gw = (int)((block_rows < R + 31 ? block_rows : (R + 31) / 32 * 32) / 32);
  const int P = ds2_cdiv(ds2_cdiv(R, 32), gw);
  const dim3 grid_x(ds2_cdiv(ds2_cdiv(R, 32), gx), ds2_cdiv(H, 64)), grid_w(P, ds2_cdiv(H, 32));
  if (Cp == 32) {
    hipLaunchKernelGGL(k_fc_dw<1>, grid_w, dim3(64), 0, st, dlogits, ldg, (const uint16_t*)Xh, ldx, ws, (int)R, H, gw);
    DS2_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_fc_dx<1>, grid_x, dim3(64), 0, st, dlogits, ldg, (const uint16_t*)Wp, ldw, (uint16_t*)dXh, lddx, (int)R, H, gx);
  } else {
    hipLaunchKernelGGL(k_fc_dw<2>, grid_w, dim3(64), 0, st, dlogits, ldg, (const uint16_t*)Xh, ldx, ws, (int)R, H, gw);
    DS2_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_fc_dx<2>, grid_x, dim3(64), 0, st, dlogits, ldg, (const uint16_t*)Wp, ldw, (uint16_t*)dXh, lddx, (int)R, H, gx);
  }
  DS2_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_fc_sum_partials, dim3(ds2_cdiv((long)Cp * H, 256)), dim3(256), 0, st, (const float*)ws, dW, Cp * H, P);
  DS2_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
