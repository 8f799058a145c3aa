// Head of the scratch (`ws`) of a persistent recurrent sweep; the exchange buffer follows it, and whatever the chosen kernel family
// keeps behind that (ds2_rnn_persist.hip, Plan).  Head, exchange buffer and tail are reset to 0xFF bytes before every launch: the
// payload-only exchanges use the all-ones dword as "not published yet"; an all-ones tag never equals a step index, an all-ones
// handshake slot is not a signature, the error word counts as raised only when it is 1, an all-ones spin budget is none beyond
// SPIN_LIMIT, and the arrival word counts up from all-ones.
#pragma once
#include <stddef.h>

#include "ds2_common.h"

namespace ds2p {

// The words of one launch that its workgroups share.  The kernels are handed the address of `raised` (PArgs / QArgs::lerr).
struct LaunchWords {
  int raised;        // 1: a workgroup of this launch gave up waiting; its peers stop early (raise_err, raise_err_startup)
  int spin_budget;   // polls a mid-sweep wait may take (ds2_persist_opts.spin_limit), read as unsigned (spin_check)
  unsigned arrived;  // arrival count of the kernels without an XCC-id handshake (wait_all_resident)
};
__device__ __forceinline__ LaunchWords* launch_words(int* lerr) { return reinterpret_cast<LaunchWords*>(lerr); }

constexpr long AUX_BYTES = 4096;
struct ScratchHead {
  unsigned long long probe[128];      // cycle counters of workgroup 0 of each group (-DDS2_PROBE builds only)
  unsigned long long xcc[8 * 32];     // XCC-id handshake slots of the tuned kernels: [NGROUPS][32 workgroups]
  LaunchWords lw;
  unsigned char unused[AUX_BYTES - 3072 - sizeof(LaunchWords)];
};
// the kernels' addressing: these are the offsets every round so far has used
static_assert(sizeof(ScratchHead) == AUX_BYTES, "the exchange buffer starts AUX_BYTES into the scratch");
static_assert(offsetof(ScratchHead, probe) == 0 && offsetof(ScratchHead, xcc) == 1024, "scratch head layout");
static_assert(offsetof(ScratchHead, lw) + offsetof(LaunchWords, raised) == 3072, "scratch head layout");
static_assert(offsetof(ScratchHead, lw) + offsetof(LaunchWords, spin_budget) == 3076, "scratch head layout");
static_assert(offsetof(ScratchHead, lw) + offsetof(LaunchWords, arrived) == 3080, "scratch head layout");

}  // namespace ds2p
