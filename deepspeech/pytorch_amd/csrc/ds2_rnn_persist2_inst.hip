// One row of DS2_PERSIST2_INSTANCES (ds2_rnn_persist_widths.h): the round-2 general persistent recurrent kernels
// (ds2_rnn_persist2_impl.h) of one (cell, storage type, hidden size, m-tiles).  build.py compiles this file once per row with
// -DDS2_INST=<CELL>,<T>,<H>,<MT>.
#include "ds2_rnn_persist2_impl.h"
#ifndef DS2_INST
#error "compile with -DDS2_INST=<the arguments of a row of DS2_PERSIST2_INSTANCES>"
#endif

namespace ds2q {
template int launch2<DS2_INST>(bool, const QArgs&, hipStream_t);
}  // namespace ds2q
