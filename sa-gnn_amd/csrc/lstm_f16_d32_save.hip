// Split-f16 interval LSTM, d = 32, training forward (stores gate activations and cell states).
#include "lstm_f16_kernel.h"

namespace sagnn {
int lstm_f16_d32_save(const LstmArgs& a, hipStream_t s) { return launch_lstm_f16<32, true, false>(a, s); }
}  // namespace sagnn
