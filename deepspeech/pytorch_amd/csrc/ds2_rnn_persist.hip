// Host side of the persistent recurrent sweeps: ONE routing decision (plan), from which the support queries, the scratch size and the
// launches all read.  The kernel families, by ds2_rnn_persist_kind's numbers:
//   1, 2  tuned kernels (ds2_rnn_persist_impl.h, instantiated per cell in ds2_rnn_persist_{gru,lstm,rnn}.hip): bf16, H = 1024, 8 XCD-local
//         groups of 32 workgroups, <= 8 / 9-16 samples per group -- BASELINE.json config 3;
//   3     general kernels, round 4 (ds2_rnn_persist3_impl.h): bf16, GRU / LSTM, 32 units per workgroup, XCD-local groups for H <= 1024, up
//         to 32 samples per group in two sample sets with their own step schedules -- config 5 and every bf16 width / batch the tuned
//         kernels do not take;
//   4     general kernels, round 2 (ds2_rnn_persist2_impl.h): bf16 and fp32 storage, 16 units per workgroup, up to 64 samples per group --
//         config 2 (the fp32 parity mode) and bf16 groups of > 32 samples.
// Which widths families 3 and 4 are instantiated for is ds2_rnn_persist_widths.h's to say (one object per row, ds2_rnn_persist{3,2}_inst.hip);
// the layout of the scratch head is ds2_rnn_persist_scratch.h's.
#include "ds2_rnn_persist3_impl.h"
#include "ds2_rnn_persist_scratch.h"
#include "ds2_rnn_persist_widths.h"

namespace ds2p {
int launch_gru(bool bwd, int H, const PArgs& a, hipStream_t st);
int launch_lstm(bool bwd, int H, const PArgs& a, hipStream_t st);
int launch_rnn(bool bwd, int H, const PArgs& a, hipStream_t st);
}  // namespace ds2p
namespace ds2r {
#define DS2_ROW(HH)                                                                         \
  extern template int launch3<CELL_GRU, HH>(bool, bool, const RArgs&, hipStream_t); \
  extern template int launch3<CELL_LSTM, HH>(bool, bool, const RArgs&, hipStream_t);
DS2_PERSIST3_WIDTHS(DS2_ROW)
#undef DS2_ROW
}  // namespace ds2r
namespace ds2q {
#define DS2_ROW(CELL, T, HH, M) extern template int launch2<CELL, T, HH, M>(bool, const QArgs&, hipStream_t);
DS2_PERSIST2_INSTANCES(DS2_ROW)
#undef DS2_ROW
}  // namespace ds2q

namespace {
using namespace ds2p;
using ds2q::QArgs;
using ds2r::RArgs;

int cu_count() {   // of the CURRENT device (cached per device)
  static int n[DS2_MAX_DEVICES];
  int dev = 0, v = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= DS2_MAX_DEVICES) return 0;
  if (n[dev] == 0 && hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess) n[dev] = v;
  return n[dev];
}

// How long the workgroups of a launch wait for ALL of them to become resident (csrc/ds2_rnn_persist_impl.h, raise_err_startup).
constexpr unsigned STARTUP_MS_DEFAULT = 300;
unsigned startup_ms(const ds2_persist_opts* o) { return o && o->startup_ms ? o->startup_ms : STARTUP_MS_DEFAULT; }
unsigned variant_of(const ds2_persist_opts* o) { return o ? o->variant : 0u; }

int gates(int cell) { return cell == CELL_GRU ? 3 : cell == CELL_LSTM ? 4 : 1; }

int launch1_any(bool bwd, int cell, int H, const PArgs& a, hipStream_t st) {
  switch (cell) {
    case CELL_GRU: return launch_gru(bwd, H, a, st);
    case CELL_LSTM: return launch_lstm(bwd, H, a, st);
    case CELL_RNN: return launch_rnn(bwd, H, a, st);
  }
  return DS2_ERR_ARG;
}
// 0 on success, DS2_ERR_ARG if the combination is not instantiated; `probe` only asks whether it is
int launch3_any(bool probe, bool bwd, int cell, int H, const RArgs& a, hipStream_t st) {
  if (cell != CELL_GRU && cell != CELL_LSTM) return DS2_ERR_ARG;
#define DS2_ROW(HH) \
  if (H == HH) return cell == CELL_GRU ? ds2r::launch3<CELL_GRU, HH>(probe, bwd, a, st) : ds2r::launch3<CELL_LSTM, HH>(probe, bwd, a, st);
  DS2_PERSIST3_WIDTHS(DS2_ROW)
#undef DS2_ROW
  return DS2_ERR_ARG;
}
bool inst3(int cell, int H, int sparse) {
  RArgs dummy{};
  dummy.sparse = sparse;
  return launch3_any(true, false, cell, H, dummy, nullptr) == 0;
}
template <typename T>
constexpr int dtype_of = std::is_same<T, float>::value ? DS2_F32 : DS2_BF16;
int launch2_any(bool probe, bool bwd, int dtype, int cell, int H, int MT, const QArgs& a, hipStream_t st) {
#define DS2_ROW(CELL, T, HH, M) \
  if (dtype == dtype_of<T> && cell == CELL && H == HH && MT == M) return probe ? 0 : ds2q::launch2<CELL, T, HH, M>(bwd, a, st);
  DS2_PERSIST2_INSTANCES(DS2_ROW)
#undef DS2_ROW
  return DS2_ERR_ARG;
}

// The routing decision for one problem: which family runs it, that family's geometry, and its scratch.
struct Plan {
  int family;                  // 0 none, 1 / 2 tuned (<= 8 / 9-16 samples per group), 3 round-4 general, 4 round-2 general
  int gpd, NG, P;              // groups per direction, groups (gpd * D), workgroups per group
  int MT;                      // family 4: m-tiles of 16 samples per group
  int xmap, gx, nset, sparse;  // family 3: RArgs' fields of these names
  long xbuf_fwd, xbuf_bwd;     // exchange buffer of a forward / a BPTT sweep (behind the head)
  long tail_bytes;             // what follows the sweep's exchange buffer and is reset with it: family 3's XCC-id handshake words
  long probe_bytes;            // -DDS2_PROBE builds, tuned kernels: the step timeline at the very end of the scratch (never reset)
  long xbuf(bool bwd) const { return bwd ? xbuf_bwd : xbuf_fwd; }
  long reset_bytes(bool bwd) const { return AUX_BYTES + xbuf(bwd) + tail_bytes; }
  long ws_bytes() const { return family ? reset_bytes(true) + probe_bytes : 0; }   // BPTT exchanges G * H values per sample, forward H
};

// Routing bits (ds2_persist_opts.variant / the `variant` argument of the queries; 0 = the shipping routing), by which the tests and the
// probe tools reach a family on shapes that the default routing sends elsewhere: bit 0 (1) = do not use the round-4 general kernels;
// bit 3 (8) = the general kernels take H = 1024 too; bit 4 (16) = the tuned kernels keep 9-16 clips per group.  Any other bit is a
// caller's mistake: no family, and the sweeps answer DS2_ERR_ARG.  The bits travel with every call (and so does the spin budget), so
// the entries are re-entrant and a test that dies cannot re-route the launches after it.
//
// cus = compute units to plan for: the device's, or 256 for "would a full device take this shape".  Arithmetic and the instantiation
// tables only -- no HIP call.  Every family wants one workgroup per CU and all of them co-resident, hence >= 256 CUs.
constexpr unsigned VARIANT_LIVE = 1u | 8u | 16u;
bool plan(int dtype, int cell, int D, int N, int H, int cus, unsigned variant, Plan& pl) {
  pl = Plan{};
  if (variant & ~VARIANT_LIVE) return false;
  if ((cell != CELL_GRU && cell != CELL_LSTM && cell != CELL_RNN) || (D != 1 && D != 2) || N < 1 || cus < 256) return false;
  const bool bf16 = dtype == DS2_BF16;
  const long kf = H, kb = (long)gates(cell) * H;   // K of the recurrent product: forward, BPTT
  auto ceil_div = [](int a, int b) { return (a + b - 1) / b; };

  // tuned kernels.  Bit 3: the general kernels take H = 1024 too.  9-16 clips per group: the round-4 general kernels are faster (GRU bi,
  // 64 clips: 2.7 vs 3.4 us per forward step, profiles/r04n_time_sweeps.txt) unless bit 4 asks for the tuned ones; RNN cells only exist here
  if (bf16 && H == 1024 && !(variant & 8u)) {
    const int ns = ceil_div(N, NGROUPS / D);
    if (ns <= (((variant & 16u) || cell == CELL_RNN) ? MAXS : 8)) {
      pl.family = ns <= 8 ? 1 : 2;
      pl.gpd = NGROUPS / D, pl.NG = NGROUPS, pl.P = 32;
      pl.xbuf_fwd = (long)NGROUPS * 2 * MAXS * (kf / 2) * 8;
      pl.xbuf_bwd = (long)NGROUPS * 2 * MAXS * (kb / 2) * 8;
#ifdef DS2_PROBE
      pl.probe_bytes = 32 * TL_N * TL_K * 8;
#endif
      return true;
    }
  }

  // round-4 general kernels: P = H / 32 workgroups per group
  if (!(variant & 1u) && bf16 && H % 32 == 0 && (cell == CELL_GRU || cell == CELL_LSTM)) {
    pl.P = H / 32;
    pl.xmap = pl.P <= 32;   // a group fits one XCD: 8 x floor(32 / P) group slots, block b on XCD b % 8
    pl.gx = pl.xmap ? 32 / pl.P : 0;
    pl.gpd = (pl.xmap ? 8 * pl.gx : 256 / pl.P) / D;
    if (pl.gpd > N) pl.gpd = N;
    const int ns = pl.gpd ? ceil_div(N, pl.gpd) : 0;
    // groups of <= 8 clips: ONE set on the structured-sparse products where the width has them (H % 256 == 0).  9-16 clips stay one
    // dense 16-row set: as two sparse sets of <= 8 they lose, a half-step is a latency chain whatever its matrix work -- config 5b's
    // groups of 11: 4.07 / 4.54 us per time step against 2.71 / 3.38 (profiles/r06c_time_sweeps.txt).  From H = 1024 on
    // (profiles/r06e_sparse_single_set.txt): LSTM-1280, 8 clips per group 2.62 / 2.88 against 2.70 / 3.01 us per time step dense;
    // GRU-768 equal; LSTM-512 forward 1.93 against 1.69 (two k-blocks per wave leave nothing to overlap)
    pl.sparse = ns <= 8 && H >= 1024 && inst3(cell, H, 1);
    pl.nset = ns <= 16 ? 1 : ns <= 32 ? 2 : 0;
    if (pl.gpd >= 1 && pl.nset && inst3(cell, H, 0)) {
      pl.family = 3;
      pl.NG = pl.gpd * D;
      // per group: nset sets x four payload slots of [k-step][lq][16 rows] x 16 B
      pl.xbuf_fwd = (long)pl.NG * pl.nset * 4 * (kf / 32) * 1024;
      pl.xbuf_bwd = (long)pl.NG * pl.nset * 4 * (kb / 32) * 1024;
      // XCC-id handshake words, 32 per group, BEHIND the exchange buffer: up to 32 groups (8 x gx) do not fit the 2 KB the tuned
      // kernels' eight groups use inside the head -- with 16 groups (H = 512) the words of groups 8-15 used to land on the spin budget
      // and on the first group's exchange slots (an intermittent stale read at the second time step)
      pl.tail_bytes = (long)pl.NG * 32 * 8;
      return true;
    }
    pl = Plan{};
  }

  // round-2 general kernels: P = H / 16 workgroups per group, as many groups per direction as the chip holds
  if ((!bf16 && dtype != DS2_F32) || H % 16 != 0 || H / 16 * D > cus) return false;
  pl.P = H / 16;
  pl.gpd = cus / pl.P / D;
  if (pl.gpd > N) pl.gpd = N;
  const int ns = ceil_div(N, pl.gpd);
  pl.MT = ns <= 16 ? 1 : ns <= 32 ? 2 : ns <= 64 ? 4 : 0;
  if (pl.MT == 0 || launch2_any(true, false, dtype, cell, H, pl.MT, QArgs{}, nullptr) != 0) return false;
  pl.family = 4;
  pl.NG = pl.gpd * D;
  // two parities of tagged granules (2048 B per k-step and m-tile) or four payload-only slots (1024 B): the same bytes
  const int ksz = bf16 ? 32 : 16;
  pl.xbuf_fwd = (long)pl.NG * 2 * (kf / ksz) * pl.MT * 2048;
  pl.xbuf_bwd = (long)pl.NG * 2 * (kb / ksz) * pl.MT * 2048;
  return true;
}

// What the forward and the BPTT entry are given alike.
struct Sweep {
  bool bwd;
  int D, N, Tp;
  const int* lens;
  const void* W;      // W_hh forward, W_hh^T BPTT
  void* Hseq;
  long hseq_dstride;
  void* S;
  void* ws;
  int* err;
  const ds2_persist_opts* opts;
  hipStream_t st;
};

// Argument check, routing, reset of head + exchange buffer + tail (0xFF bytes: ds2_rnn_persist_scratch.h), the launch's spin budget.
int begin_sweep(const Sweep& s, int dtype, int cell, int H, Plan& pl) {
  DS2_REQUIRE(s.Tp > 0 && s.Tp < (int)TAG_INIT && s.ws && s.err, DS2_ERR_ARG);
  DS2_REQUIRE(plan(dtype, cell, s.D, s.N, H, cu_count(), variant_of(s.opts), pl), DS2_ERR_ARG);
  hipError_t e = hipMemsetAsync(s.ws, 0xff, pl.reset_bytes(s.bwd), s.st);
  if (e != hipSuccess || !s.opts || s.opts->spin_limit == 0) return (int)e;
  return (int)hipMemsetD32Async((hipDeviceptr_t)&static_cast<ScratchHead*>(s.ws)->lw.spin_budget, (int)s.opts->spin_limit, 1, s.st);
}

// -DDS2_PROBE builds (tools/probe_rnn_persist.py, tools/probe_persist3.py): cycle counters, work-skipping masks, step timeline
template <class A>
void probe_hooks(A& a, const Sweep& s, const Plan& pl) {
#ifdef DS2_PROBE
  a.dbg = static_cast<ScratchHead*>(s.ws)->probe;
  const char* e = getenv("DS2_PERSIST_DBG");
  a.dbgmask = e ? atoi(e) : 0;
  if constexpr (std::is_same<A, PArgs>::value) a.tl = (unsigned long long*)((char*)s.ws + pl.ws_bytes() - pl.probe_bytes);
#endif
}

// The fields of the kernels' arguments that both directions fill the same way; the entries add their own tensors.
template <class A>
void common_args(A& a, const Sweep& s, const Plan& pl) {
  typedef decltype(a.Hseq) act_t;   // bf16_t* (PArgs) or void* (QArgs)
  a.N = s.N, a.Tp = s.Tp, a.D = s.D, a.gpd = pl.gpd, a.lens = s.lens;
  a.W = (decltype(a.W))s.W, a.Hseq = (act_t)s.Hseq, a.hseq_dstride = s.hseq_dstride, a.S = (act_t)s.S;
  a.xbuf = (decltype(a.xbuf))((char*)s.ws + AUX_BYTES);
  a.err = s.err, a.lerr = &static_cast<ScratchHead*>(s.ws)->lw.raised, a.startup_ms = startup_ms(s.opts);
}
PArgs pargs(const Sweep& s, const Plan& pl) {
  PArgs a{};
  common_args(a, s, pl);
  a.xcc = static_cast<ScratchHead*>(s.ws)->xcc;
  probe_hooks(a, s, pl);
  return a;
}
QArgs qargs(const Sweep& s, const Plan& pl) {
  QArgs a{};
  common_args(a, s, pl);
  a.NG = pl.NG, a.xgroup_bytes = pl.xbuf(s.bwd) / pl.NG;
  return a;
}
RArgs rargs(const Sweep& s, const Plan& pl) {
  RArgs ra{};
  ra.q = qargs(s, pl);
  ra.xcc = (u64*)((char*)s.ws + AUX_BYTES + pl.xbuf(s.bwd));
  ra.P = pl.P, ra.xmap = pl.xmap, ra.gx = pl.gx, ra.nset = pl.nset, ra.sparse = pl.sparse;
  ra.skip = pl.nset == 2;
  probe_hooks(ra, s, pl);
  return ra;
}

// Two-set groups execute a set's half-steps only while one of its clips is inside its sequence (ds2r::sched3): the padding rows of
// the sweep's outputs are zeroed here instead of by the half-steps left out.  One workgroup per 4 rows of a [T' x N] matrix.
__global__ void __launch_bounds__(256) k_zero_pad3(unsigned char* X, long ld_bytes, int row_bytes, const int* __restrict__ lens, int N, long R) {
  const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= R) return;
  if ((int)(r / N) < lens[r % N]) return;
  unsigned char* p = X + r * ld_bytes;
  for (int o = (threadIdx.x & 63) * 16; o < row_bytes; o += 64 * 16) *reinterpret_cast<uint4*>(p + o) = make_uint4(0, 0, 0, 0);
}
void zero_pad3(void* X, long ld_bytes, long row_bytes, const Sweep& s) {
  const long R = (long)s.Tp * s.N;
  hipLaunchKernelGGL(k_zero_pad3, dim3((unsigned)((R + 3) / 4)), dim3(256), 0, s.st, (unsigned char*)X, ld_bytes, (int)row_bytes, s.lens, s.N, R);
}

}  // namespace

extern "C" {

// The routing decision with the CU count given: family (ds2_rnn_persist_kind's numbers) and, if ws_bytes is not null, the scratch bytes
// of one sweep (head + the larger, BPTT, exchange buffer + tail).  No device is asked: host tests pin the routing table through it.
int ds2_rnn_persist_plan(int dtype, int cell, int D, int N, int H, int cus, unsigned variant, long* ws_bytes) {
  Plan pl;
  plan(dtype, cell, D, N, H, cus, variant, pl);
  if (ws_bytes) *ws_bytes = pl.ws_bytes();
  return pl.family;
}

// 1 if a persistent kernel covers this problem on the current device (>= 256 CUs: one workgroup per CU, all co-resident).
int ds2_rnn_persist_supported(int dtype, int cell, int D, int N, int H, unsigned variant) {
  return ds2_rnn_persist_plan(dtype, cell, D, N, H, cu_count(), variant, nullptr) != 0;
}

// Which kernel family ds2_rnn_persist_fwd / _bwd run for the problem on the current device: 0 none, 1 tuned (H = 1024, <= 8 samples
// per group: k_rnn_persist_fwd4 / bwd4), 2 tuned (9-16 samples: k_rnn_persist_fwd / bwd), 3 round-4 general (k_rnn_persist3_*),
// 4 round-2 general (k_rnn_persist2_*).  For measurement tools (bench.py names the rocprofv3 kernel from it).
int ds2_rnn_persist_kind(int dtype, int cell, int D, int N, int H, unsigned variant) {
  return ds2_rnn_persist_plan(dtype, cell, D, N, H, cu_count(), variant, nullptr);
}

// 1 if a persistent kernel is INSTANTIATED for this problem, whatever the current device's CU count (what a full 256-CU device
// would run): lets the caller tell "this device is too small" (an error) from "no persistent kernel for this shape" (a warning).
int ds2_rnn_persist_shape_covered(int dtype, int cell, int D, int N, int H) {
  return ds2_rnn_persist_plan(dtype, cell, D, N, H, 256, 0u, nullptr) != 0;
}

long ds2_rnn_persist_ws_bytes(int dtype, int cell, int D, int N, int H, unsigned variant) {
  long bytes = 0;
  ds2_rnn_persist_plan(dtype, cell, D, N, H, cu_count(), variant, &bytes);
  return bytes;
}

// Same contract as ds2_rnn_fwd (ds2_rnn.hip); ws = ds2_rnn_persist_ws_bytes() bytes (reset here).
// err: one device int, set to 1 if a workgroup gave up waiting (outputs are then NaN-poisoned).
int ds2_rnn_persist_fwd(int dtype, int cell, int D, int N, int H, int Tp, const int* lens, const void* GI, const void* Whh,
                        const float* bhh, const float* h0, const float* c0, void* Hseq, long hseq_dstride, void* S, float* hn,
                        float* cn, void* ws, int* err, const ds2_persist_opts* opts, ds2_stream_t st_) {
  const Sweep s{false, D, N, Tp, lens, Whh, Hseq, hseq_dstride, S, ws, err, opts, (hipStream_t)st_};
  Plan pl;
  if (int r = begin_sweep(s, dtype, cell, H, pl)) return r;
  auto inputs = [&](auto& a) {
    a.bhh = bhh, a.GI = (decltype(a.GI))GI, a.h0 = h0, a.c0 = c0, a.hn = hn, a.cn = cn;
  };
  if (pl.family <= 2) {
    PArgs a = pargs(s, pl);
    inputs(a);
    return launch1_any(false, cell, H, a, s.st);
  }
  if (pl.family == 4) {
    QArgs a = qargs(s, pl);
    inputs(a);
    return launch2_any(false, false, dtype, cell, H, pl.MT, a, s.st);
  }
  RArgs ra = rargs(s, pl);
  inputs(ra.q);
  if (ra.skip)
    for (int d = 0; d < D; ++d)       // h_t of the padding frames (Hseq points at t = 0)
      zero_pad3((char*)Hseq + (long)d * hseq_dstride * 2, (long)H * 2, (long)H * 2, s);
  return launch3_any(false, false, cell, H, ra, s.st);
}

// BPTT sweep.  Inputs as ds2_rnn_bwd (zero initial state).  Outputs: dGI [Tp*N][D*G*H]; for GRU dQ [D][Tp][N][H] = dn * r, the
// only slot of the hidden-side gate gradient that differs from dGI's (d(W_hh h + b_hh) = [dr, dz, dQ]); dBacc [D][N][NB*H] f32
// (may be null) = per-sample sums over time of the gate-gradient planes as stored (NB = 4 for GRU: dr, dz, dn, dQ; G otherwise):
// bias_ih.grad = sum over samples of planes 0..G-1, bias_hh.grad (GRU) = planes 0, 1, 3.
int ds2_rnn_persist_bwd(int dtype, int cell, int D, int N, int H, int Tp, const int* lens, const void* dOut, const void* WhhT,
                        const void* Hseq, long hseq_dstride, const void* S, void* dGI, void* dQ, float* dBacc, int flags, void* ws,
                        int* err, const ds2_persist_opts* opts, ds2_stream_t st_) {
  const Sweep s{true, D, N, Tp, lens, WhhT, (void*)Hseq, hseq_dstride, (void*)S, ws, err, opts, (hipStream_t)st_};
  DS2_REQUIRE(cell != CELL_GRU || dQ != nullptr, DS2_ERR_ARG);
  Plan pl;
  if (int r = begin_sweep(s, dtype, cell, H, pl)) return r;
  auto gradients = [&](auto& a) {
    a.dOut = (decltype(a.dOut))dOut, a.dGI = (decltype(a.dGI))dGI, a.dGH = (decltype(a.dGH))dQ, a.dBacc = dBacc;
  };
  if (pl.family <= 2) {
    PArgs a = pargs(s, pl);
    gradients(a);
    return launch1_any(true, cell, H, a, s.st);
  }
  if (pl.family == 4) {
    QArgs a = qargs(s, pl);
    gradients(a);
    return launch2_any(false, true, dtype, cell, H, pl.MT, a, s.st);
  }
  RArgs ra = rargs(s, pl);
  gradients(ra.q);
  if (ra.skip && !(flags & 1)) {     // flags bit 0: nobody reads the padding rows (row-list consumers)
    const long GHb = (long)gates(cell) * H * 2;
    zero_pad3(dGI, D * GHb, D * GHb, s);
    if (dQ)
      for (int d = 0; d < D; ++d) zero_pad3((char*)dQ + (long)d * Tp * N * H * 2, (long)H * 2, (long)H * 2, s);
  }
  return launch3_any(false, true, cell, H, ra, s.st);
}

}  // extern "C"
