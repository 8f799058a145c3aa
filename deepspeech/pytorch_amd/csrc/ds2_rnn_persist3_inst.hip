// One row of DS2_PERSIST3_WIDTHS (ds2_rnn_persist_widths.h): the round-4 general persistent recurrent kernels
// (ds2_rnn_persist3_impl.h) of hidden size DS2_INST, GRU and LSTM.  build.py compiles this file once per row with -DDS2_INST=<H>.
#include "ds2_rnn_persist3_impl.h"
#ifndef DS2_INST
#error "compile with -DDS2_INST=<a hidden size of DS2_PERSIST3_WIDTHS>"
#endif

namespace ds2r {
template int launch3<CELL_GRU, DS2_INST>(bool, bool, const RArgs&, hipStream_t);
template int launch3<CELL_LSTM, DS2_INST>(bool, bool, const RArgs&, hipStream_t);
}  // namespace ds2r
