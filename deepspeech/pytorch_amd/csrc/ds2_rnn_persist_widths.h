// The instantiation tables of the general persistent recurrent kernels -- the ONE list of widths.  Adding a width is one row here:
//   * ds2_rnn_persist.hip generates its declarations and launch3_any / launch2_any from these tables;
//   * build.py compiles ds2_rnn_persist3_inst.hip / ds2_rnn_persist2_inst.hip once per row, the row's arguments passed as
//     -DDS2_INST=<arguments> (one object per row keeps hipcc's time per file bounded and the build parallel).  It reads the rows with a
//     regular expression: keep every row on one line, in the form X(<arguments>), and write X( in this file for nothing else;
//   * ops.use_persistent and model._padded_hidden ask ds2_rnn_persist_shape_covered, which asks the same tables.
// The tuned kernels (ds2_rnn_persist_impl.h) exist for H = 1024 alone and are not listed.
#pragma once

// Round-4 general kernels (ds2_rnn_persist3_impl.h: bf16 storage, 32 hidden units per workgroup): one row per hidden size, GRU and LSTM
// each where covered3<CELL, H>() finds a register / LDS plan (LSTM: not 1408 / 1536).  512, 768, 800, 1024, 1280, 1536 are round 4's
// (BASELINE config 5 and every bf16 width / batch the tuned kernels do not take); round 5 added the widths between them, so that every
// bf16 hidden size up to 1536 reaches a persistent kernel after at most 128 units of zero padding (model.DeepSpeech._padded_hidden).
#define DS2_PERSIST3_WIDTHS(X) \
  X(384)                       \
  X(512)                       \
  X(640)                       \
  X(768)                       \
  X(800)                       \
  X(896)                       \
  X(1024)                      \
  X(1152)                      \
  X(1280)                      \
  X(1408)                      \
  X(1536)

// Round-2 general kernels (ds2_rnn_persist2_impl.h: 16 hidden units per workgroup): one row per (cell, storage type, hidden size,
// m-tiles of 16 clips per group).  The m-tile counts are the ones the BASELINE configurations need (cfg2: 1, cfg5b: 2, cfg5a: 4); the
// fp32 tanh cells are round 6's (the fp32 mode had them on one launch per time step).
#define DS2_PERSIST2_INSTANCES(X) \
  X(CELL_GRU, bf16_t, 800, 1)     \
  X(CELL_LSTM, bf16_t, 800, 1)    \
  X(CELL_GRU, bf16_t, 1280, 1)    \
  X(CELL_LSTM, bf16_t, 1280, 1)   \
  X(CELL_GRU, bf16_t, 1280, 2)    \
  X(CELL_LSTM, bf16_t, 1280, 2)   \
  X(CELL_GRU, bf16_t, 1280, 4)    \
  X(CELL_LSTM, bf16_t, 1280, 4)   \
  X(CELL_GRU, float, 800, 1)      \
  X(CELL_LSTM, float, 800, 1)     \
  X(CELL_RNN, float, 800, 1)      \
  X(CELL_GRU, float, 1024, 1)     \
  X(CELL_LSTM, float, 1024, 1)    \
  X(CELL_RNN, float, 1024, 1)     \
  X(CELL_GRU, float, 1280, 1)     \
  X(CELL_LSTM, float, 1280, 1)    \
  X(CELL_RNN, float, 1280, 1)
