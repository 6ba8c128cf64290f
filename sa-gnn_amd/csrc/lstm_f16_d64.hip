// Split-f16 interval LSTM, d = 64, inference (with and without an output-dropout mask).
#include "lstm_f16_kernel.h"

namespace sagnn {
int lstm_f16_d64(const LstmArgs& a, hipStream_t s) {
  if (a.drop) return launch_lstm_f16<64, false, true>(a, s);
  return launch_lstm_f16<64, false, false>(a, s);
}
}  // namespace sagnn
