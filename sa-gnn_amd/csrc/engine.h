// Kernel selection of the fusion stages: the calling thread's engine and one pure selector per stage. Each selector
// takes the engine as a parameter with the shape and alignment facts it needs and names the implementation to run;
// the C entries validate, select and switch. engine.cpp holds the selectors and the table they implement.
#pragma once
#include <stdint.h>

#include "sagnn.h"

namespace sagnn {

enum class Engine { F16x2 = SAGNN_ENGINE_F16X2, F32 = SAGNN_ENGINE_F32, Valu = SAGNN_ENGINE_VALU };
Engine calling_engine();   // sagnn_set_engine of this thread; F16x2 on a thread that never set one

enum class LstmFwd { F16x2, F32Mfma, Split128, Valu };
enum class AttnFwd { Split, F32Mfma, Wide, Valu };
enum class AttnBwdFront { Split, F32Mfma, None };
enum class AttnBwdTail { F16x2, F32Mfma, None };
enum class LstmBwd { OneLaunch, SplitDw, None };   // SplitDw: BPTT without dW, then dW on the f16 engine (lstm_dw_f16)

// vec: x (and h_init) rows 16-byte aligned; h_vec: h too; drop_vec: the mask is absent or 16-byte aligned
LstmFwd select_lstm_fwd(Engine e, int d, int t, bool vec, int64_t ld_h, bool h_vec, bool train, bool drop, bool drop_vec);
AttnFwd select_attn_fwd(Engine e, int d, int t, int heads, bool vec);
AttnBwdFront select_attn_bwd_front(Engine e, int d, int t, int heads);
AttnBwdTail select_attn_bwd_tail(Engine e, int d);
LstmBwd select_lstm_bwd(Engine e, int d, bool workspace);

// shapes the kernel families cover; the launchers check them too
bool mhsa_split_supported(int d, int t, int heads);             // attn_split.hip, forward
bool attn_bwd_front_split_supported(int d, int t, int heads);   // attn_split.hip, backward front
bool mhsa_mfma_supported(int d, int t, int heads);              // fusion_mfma.hip
bool wide_supported(int d);                                     // fusion.hip, mhsa_mean_wide

}  // namespace sagnn
