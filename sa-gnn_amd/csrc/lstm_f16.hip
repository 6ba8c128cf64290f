// Dispatcher of the split-f16 interval LSTM (kernel: lstm_f16_kernel.h; instantiations: lstm_f16_d*.hip).
#include "lstm_f16_kernel.h"

namespace sagnn {

int lstm_fwd_f16(const LstmArgs& a, hipStream_t s) {
  const bool save = a.gates != nullptr;
  const int d = a.x.d;
  // the tile's rows are addressed with 32-bit byte offsets from a per-tile base
  if (a.ld_h >= (1 << 22) || (int64_t)a.x.t * d >= (1 << 18))
    return fail(SAGNN_ERR_ARG, "f16 LSTM: output row stride must stay below 2^22 floats and t*d below 2^18");
  if (a.ld_h < (int64_t)a.x.t * d) return fail(SAGNN_ERR_ARG, "f16 LSTM: ld_h = %lld < t*d", (long long)a.ld_h);
  if (save && a.drop) return fail(SAGNN_ERR_ARG, "f16 LSTM: the training forward takes no dropout mask");
  if (d == 64) return save ? lstm_f16_d64_save(a, s) : lstm_f16_d64(a, s);
  if (d == 32) return save ? lstm_f16_d32_save(a, s) : lstm_f16_d32(a, s);
  return fail(SAGNN_ERR_DIM, "f16 LSTM supports d = 32 or 64, got %d", d);
}

}  // namespace sagnn
